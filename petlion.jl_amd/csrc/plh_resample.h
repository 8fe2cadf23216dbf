// plh_resample.h -- plh_resample: the saved points of an ensemble on ONE time grid shared by all cells (reference sol(t) / simulate(p, tf::Vector): an interpolating
// cubic spline through each run's saved points, Dierckx Spline1D with s = 0, src/save_outputs.jl:74-133).  Post-interpolation of what plh_integrate wrote: nothing here
// knows a model variant, so the kernels belong to the host translation unit (petlion_hip.hip includes this file; the wave-emulator build compiles them too).
//
// Per (cell, run) with n >= 4 points the spline is FITPACK's for k = 3, s = 0: the not-a-knot cubic (knots = the data sites but the second and the second-to-last).  It is
// computed in slope form -- unknowns s_i = S'(x_i), h_i = x_{i+1} - x_i, d_i = (y_{i+1} - y_i) / h_i:
//   row 0      h_1 s_0 + (h_0 + h_1) s_1                       = ((3 h_0 + 2 h_1) h_1 d_0 + h_0^2 d_1) / (h_0 + h_1)          (de Boor's not-a-knot row)
//   row i      h_i s_{i-1} + 2 (h_{i-1} + h_i) s_i + h_{i-1} s_{i+1} = 3 (h_i d_{i-1} + h_{i-1} d_i)
//   row n-1    the mirror of row 0
// solved by Thomas elimination without pivoting (the pivots are h_1, h_0 + h_1, then more than 2 h_{i-1} + h_i: positive), evaluated in Hermite form on the bracketing
// interval, expanded about the NEARER node: a query at a saved time returns the saved value itself.  n = 3: the parabola through the points, n = 2: the line (both as
// Hermite data: the same evaluation), n = 1: the constant -- the degrees Solution.__call__ (api.py) takes for short runs.
//
// Three kernels per chunk of cells, queued on the caller's stream:
//   k_resample_prep    one lane per cell: may the cell be resampled (status), where do its runs start, and the elimination of every run's matrix -- multiplier w_i and pivot p_i
//                      per row, which depend on t only and are shared by every column of every field
//   k_resample_locate  one lane per (cell, query): run of the query (the reference's rule), clamped query time, left node of the bracketing interval
//   k_resample_field   one wave per (cell, tile of 64 consecutive columns), lanes = columns: forward sweep (right-hand sides from src), back substitution (slopes, in the
//                      workspace), then every query.  Every load of src / the slopes and every store of dst is one contiguous row segment of <= 512 B; a lane only ever reads
//                      slopes it wrote itself, so the kernel needs no synchronisation.
#pragma once

#ifndef PL_LAUNCH
#define PL_LAUNCH(kernel, grid, block, stream, ...) hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__)
#endif

namespace plrs {

constexpr int TILE = 64;      // columns per wave

// the workspace of one chunk of cells (device memory of the stream's context; sizes in the order of the members)
struct Work {
  int* ok;            // [chunk]                  1: resample the cell, 0: NaN row
  int* run0;          // [chunk][n_runs]          first saved row of every run
  double* fac;        // [chunk][max_pts][2]      (w_i, p_i) of the row of saved point i in its run's matrix (runs with >= 4 points)
  int* loc_i;         // [chunk][n_q]             left node of the query's interval (row of the cell); ~row: the run has one point, the value is that row's
  double* loc_t;      // [chunk][n_q]             the query time after clamping (NaN: the result is NaN)
  double* slope;      // [chunk][max_pts][width]  S'(x_i) per column (the forward sweep parks its right-hand sides here)
};
__host__ __device__ inline size_t work_bytes_per_cell(int n_runs, int max_pts, int n_q, int width) {
  return sizeof(int) * (2 + (size_t)n_runs + (size_t)n_q + 1) + sizeof(double) * ((size_t)max_pts * 2 + (size_t)n_q + (size_t)max_pts * width) + 64;
}

struct Args {
  int cell0, n_chunk;                       // the cells [cell0, cell0 + n_chunk) of the call
  int n_runs, max_pts, width, n_q, extrapolate;
  const double* t; const int* n_pts; const plh_run_info* run_info; const double* src; const double* tq;
  double* dst; int* status;
  Work w;
};

__host__ __device__ inline double rs_nan() { return __builtin_nan(""); }

// ---- one lane per cell ----
__global__ void k_resample_prep(Args a) {
  const int lc = (int)(blockIdx.x * (unsigned)TILE + threadIdx.x);
  if (lc >= a.n_chunk) return;
  const size_t cell = (size_t)a.cell0 + lc;
  const plh_run_info* ri = a.run_info + cell * a.n_runs;
  int* run0 = a.w.run0 + (size_t)lc * a.n_runs;
  // a cell whose protocol failed (flag < 0: PLH_ERR_*, PLH_ERR_OUTPUT_FULL among them, or a run that never ended), whose point count is not the sum of its runs'
  // (truncated at max_pts), or with a run without a point: none of its points is read
  bool ok = true; long long sum = 0;
  for (int r = 0; r < a.n_runs; r++) {
    run0[r] = (int)(sum < a.max_pts ? sum : 0);
    if (ri[r].flag < 0 || ri[r].iterations < 1) ok = false;
    sum += ri[r].iterations > 0 ? ri[r].iterations : 0;
  }
  if (sum != (long long)a.n_pts[cell] || sum > (long long)a.max_pts) ok = false;
  a.w.ok[lc] = ok ? 1 : 0;
  if (a.status) a.status[cell] = ok ? 0 : 1;
  if (!ok) return;
  const double* x = a.t + cell * a.max_pts;
  double* fac = a.w.fac + (size_t)lc * a.max_pts * 2;
  for (int r = 0; r < a.n_runs; r++) {
    const int n = ri[r].iterations, s0 = run0[r];
    if (n < 4) continue;
    const double* xr = x + s0; double* f = fac + (size_t)s0 * 2;
    double hm = xr[1] - xr[0], h = xr[2] - xr[1];                 // h_{i-1}, h_i
    double p = h, c = hm + h;                                      // row 0: pivot and upper entry
    f[0] = 0.0; f[1] = p;
    for (int i = 1; i < n - 1; i++) {
      const double w = h / p;                                      // a_i = h_i
      p = 2.0 * (hm + h) - w * c; c = hm;
      f[2 * i] = w; f[2 * i + 1] = p;
      if (i < n - 2) { hm = h; h = xr[i + 2] - xr[i + 1]; }
    }
    // row n-1: (h_{n-2} + h_{n-3}) s_{n-2} + h_{n-3} s_{n-1}   (here hm = h_{n-3}, h = h_{n-2}, c = c_{n-2} = h_{n-3})
    const double w = (h + hm) / p;
    f[2 * (n - 1)] = w; f[2 * (n - 1) + 1] = hm - w * c;
  }
}

// ---- one lane per (cell, query) ----
__global__ void k_resample_locate(Args a) {
  const size_t id = (size_t)blockIdx.x * TILE + threadIdx.x;
  if (id >= (size_t)a.n_chunk * a.n_q) return;
  const int lc = (int)(id / a.n_q), q = (int)(id % a.n_q);
  if (!a.w.ok[lc]) return;
  const size_t cell = (size_t)a.cell0 + lc;
  const plh_run_info* ri = a.run_info + cell * a.n_runs;
  const double* x = a.t + cell * a.max_pts;
  double tv = a.tq[q];
  int* li = a.w.loc_i + (size_t)lc * a.n_q + q; double* lt = a.w.loc_t + (size_t)lc * a.n_q + q;
  if (!(tv == tv)) { *li = 0; *lt = rs_nan(); return; }
  // run r spans (t_end of run r-1, t_end of run r), span 0 starts at the first saved time; before the first span: run 0, else the first span that holds the query, else the last run
  int r = a.n_runs - 1;
  if (tv < x[0]) r = 0;
  else {
    double lo = x[0];
    for (int k = 0; k < a.n_runs; k++) { const double hi = ri[k].t_end; if (lo <= tv && tv <= hi) { r = k; break; } lo = hi; }
  }
  const int s0 = a.w.run0[(size_t)lc * a.n_runs + r], n = ri[r].iterations;
  if (!a.extrapolate) { const double xa = x[s0], xb = x[s0 + n - 1]; tv = tv < xa ? xa : (tv > xb ? xb : tv); }
  *lt = tv;
  if (n == 1) { *li = ~s0; return; }
  int lo = s0, hi = s0 + n - 2;                                    // the last left node with x <= tv (the first one for a query before the run's points)
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (x[mid] <= tv) lo = mid; else hi = mid - 1; }
  *li = lo;
}

// ---- one wave per (cell, tile of columns) ----
__global__ void k_resample_field(Args a) {
  const int n_tiles = (a.width + TILE - 1) / TILE;
  const int lc = (int)(blockIdx.x / (unsigned)n_tiles), col = (int)(blockIdx.x % (unsigned)n_tiles) * TILE + (int)threadIdx.x;
  if (lc >= a.n_chunk || col >= a.width) return;
  const size_t cell = (size_t)a.cell0 + lc;
  const size_t W = (size_t)a.width;
  double* dst = a.dst + cell * a.n_q * W + col;
  if (!a.w.ok[lc]) { for (int q = 0; q < a.n_q; q++) dst[(size_t)q * W] = rs_nan(); return; }
  const plh_run_info* ri = a.run_info + cell * a.n_runs;
  const double* x = a.t + cell * a.max_pts;
  const double* y = a.src + cell * a.max_pts * W + col;
  double* sl = a.w.slope + (size_t)lc * a.max_pts * W + col;
  const double* fac = a.w.fac + (size_t)lc * a.max_pts * 2;
  for (int r = 0; r < a.n_runs; r++) {
    const int n = ri[r].iterations, s0 = a.w.run0[(size_t)lc * a.n_runs + r];
    const double* xr = x + s0; const double* yr = y + (size_t)s0 * W; double* sr = sl + (size_t)s0 * W; const double* f = fac + (size_t)s0 * 2;
    if (n == 2) { const double d = (yr[W] - yr[0]) / (xr[1] - xr[0]); sr[0] = d; sr[W] = d; }
    else if (n == 3) {                                             // the parabola's slopes at its three points
      const double h0 = xr[1] - xr[0], h1 = xr[2] - xr[1], d0 = (yr[W] - yr[0]) / h0, d1 = (yr[2 * W] - yr[W]) / h1, c = (d1 - d0) / (h0 + h1);
      sr[0] = d0 - h0 * c; sr[W] = d0 + h0 * c; sr[2 * W] = d1 + h1 * c;
    } else if (n >= 4) {
      // forward sweep: g_i = rhs_i - w_i g_{i-1}, parked in the slope array
      double hm = xr[1] - xr[0], h = xr[2] - xr[1];
      double y0 = yr[0], y1 = yr[W], y2 = yr[2 * W];
      double dm = (y1 - y0) / hm, d = (y2 - y1) / h;              // d_{i-1}, d_i
      double g = ((3.0 * hm + 2.0 * h) * h * dm + hm * hm * d) / (hm + h);
      sr[0] = g;
      for (int i = 1; i < n - 1; i++) {
        g = 3.0 * (h * dm + hm * d) - f[2 * i] * g;
        sr[(size_t)i * W] = g;
        if (i < n - 2) { const double yn = yr[(size_t)(i + 2) * W]; hm = h; h = xr[i + 2] - xr[i + 1]; dm = d; d = (yn - y2) / h; y2 = yn; }
      }
      // (here hm = h_{n-3}, h = h_{n-2}, dm = d_{n-3}, d = d_{n-2})
      g = ((3.0 * h + 2.0 * hm) * hm * d + h * h * dm) / (hm + h) - f[2 * (n - 1)] * g;
      double s = g / f[2 * (n - 1) + 1];
      sr[(size_t)(n - 1) * W] = s;
      // back substitution: s_i = (g_i - c_i s_{i+1}) / p_i with c_0 = h_0 + h_1, c_i = h_{i-1}
      for (int i = n - 2; i >= 1; i--) { s = (sr[(size_t)i * W] - (xr[i] - xr[i - 1]) * s) / f[2 * i + 1]; sr[(size_t)i * W] = s; }
      s = (sr[0] - (xr[2] - xr[0]) * s) / f[1]; sr[0] = s;
    }
  }
  const int* loc_i = a.w.loc_i + (size_t)lc * a.n_q; const double* loc_t = a.w.loc_t + (size_t)lc * a.n_q;
  for (int q = 0; q < a.n_q; q++) {
    const double tv = loc_t[q]; const int i = loc_i[q];
    double v;
    if (!(tv == tv)) v = rs_nan();
    else if (i < 0) v = y[(size_t)(~i) * W];
    else {
      const double x0 = x[i], x1 = x[i + 1], h = x1 - x0, u = tv - x0, e = tv - x1;
      const double y0 = y[(size_t)i * W], y1 = y[(size_t)(i + 1) * W], s0 = sl[(size_t)i * W], s1 = sl[(size_t)(i + 1) * W];
      const double d = (y1 - y0) / h, c3 = (s0 + s1 - 2.0 * d) / (h * h);
      if (u <= -e) v = y0 + u * (s0 + u * ((3.0 * d - 2.0 * s0 - s1) / h + u * c3));            // about the left node
      else v = y1 + e * (s1 + e * ((s0 + 2.0 * s1 - 3.0 * d) / h + e * c3));                   // about the right node
    }
    dst[(size_t)q * W] = v;
  }
}

// the three launches of one chunk
inline void launch_chunk(hipStream_t st, const Args& a) {
  const int n_tiles = (a.width + TILE - 1) / TILE;
  PL_LAUNCH(k_resample_prep, (unsigned)((a.n_chunk + TILE - 1) / TILE), TILE, st, a);
  PL_LAUNCH(k_resample_locate, (unsigned)(((size_t)a.n_chunk * a.n_q + TILE - 1) / TILE), TILE, st, a);
  PL_LAUNCH(k_resample_field, (unsigned)((size_t)a.n_chunk * n_tiles), TILE, st, a);
}

}  // namespace plrs

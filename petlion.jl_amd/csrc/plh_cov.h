// plh_cov.h -- plh_fit_cov: parameter covariances and identifiability of every fitted problem (include/petlion_hip.h states the definition, sentence by sentence what
// k_fit_cov does).  Like plh_lm.h: no model variant, host translation unit.
//
//   k_fit_cov    one block = one wave = 64 consecutive problems, lanes = problems, in the house style of k_lm_step.  The k x k input (JtJ) and the three k x k outputs (cov,
//                corr, evec) move between HBM and LDS along the block's contiguous segment (lanes = segment); in LDS a matrix sits as [entry][problem] with rows padded to 65,
//                entry (i, j) in row 8 i + j whatever k is.  One instantiation per k = 1 .. 8: every loop over keys is unrolled to it, so every LDS address of the work of a
//                problem is lane + a constant and no register array is indexed at run time.  Two tiles, 2 x 33 280 B:
//                  A   C in its strict upper triangle (it stays there to the end of the Cholesky part); the lower triangle and the diagonal take the Cholesky factor L, then
//                      X = L^-1 in place (column by column), then P = X^T X in place (row by row).  Afterwards the diagonal is set back to 1 and the upper triangle with the
//                      diagonal is the Jacobi working matrix (with compile-time indices the upper triangle alone is enough).
//                  B   stages cov, then corr, for their segment stores; then it holds the eigenvectors V (V_rc in row 8 r + c), which the last segment store reads transposed.
//                Keys that are not analysed (held, unseen) are identity rows of C: their off-diagonal entries are exact zeros, the Cholesky factor keeps them zero, and Jacobi
//                never rotates an exact zero, so their columns of V stay unit vectors exactly.  The sweep loop is a per-lane loop: the wave runs until no lane rotated, lanes that
//                are done are predicated off.  The ascending sort is an unrolled network of conditional swaps of neighbouring columns of V (stable: ties keep their order).
//                No atomics, no inline assembly, no scratch; the barriers stand outside every per-lane condition.
#pragma once

#include <cfloat>

#include "plh_resample.h"

namespace plcov {

constexpr int NK = PLH_LSQ_MAX_SENS;      // keys at most
constexpr int TILE = 64;                  // problems per block = lanes
constexpr int LD = TILE + 1;              // a tile's row: 64 problems and one of padding

struct Args {
  int n, n_keys;
  int bstride;                              // lo / hi of problem c, key i: [c bstride + i] (per-cell bounds: n_keys; shared bounds: 0, the device copy of the host's [n_keys])
  unsigned logmask;                         // bit i: key i is PLH_LM_LOG
  const double* theta; const double* lo; const double* hi;      // either bound may be NULL (no bound on that side)
  const double* cost; const double* grad; const double* JtJ; const int* n_data;      // n_data may be NULL (sigma2 = 1)
  double* sigma2; double* cov; double* se; double* corr; double* eval; double* evec; double* coll;
  int* free_mask; int* status;
};

__device__ inline bool cov_finite(double x) { return fabs(x) <= DBL_MAX; }      // (false for NaN)

template <int K>                          // = n_keys
__global__ void __launch_bounds__(TILE) k_fit_cov(Args a) {
  __shared__ double A[NK * NK][LD];
  __shared__ double B[NK * NK][LD];
  constexpr int k = K, kk = K * K;
  const int lane = (int)threadIdx.x;
  const size_t p0 = (size_t)blockIdx.x * TILE, prob = p0 + lane;
  const int nb = (int)((size_t)a.n - p0 < (size_t)TILE ? (size_t)a.n - p0 : (size_t)TILE);      // problems of this block
  const bool live = lane < nb;
  const double qnan = __builtin_nan("");
  auto ent = [](int e) { return e / K * NK + e % K; };             // entry e of a k x k matrix -> its row of a tile

  // ---- JtJ -> A, lanes along the block's segment
  for (int x = lane; x < nb * kk; x += TILE) A[ent(x % kk)][x / kk] = a.JtJ[p0 * kk + x];
  __syncthreads();

  // ---- lanes = problems: the input check, the scaling, the active set, C
  bool ok = live, sing = false;
  int st = 0, fm = 0, n_an = 0;
  unsigned heldm = 0, unm = 0, anm = 0;                              // bit i: key i is held / unseen / analysed
  double s[K], r[K], sg2 = qnan;
  if (live) {
    const double cost = a.cost[prob];
    double g[K], Hd[K];
    ok = cov_finite(cost);
#pragma unroll
    for (int i = 0; i < k; i++) {
      const double th = a.theta[prob * k + i];
      const double l = a.lo ? a.lo[prob * a.bstride + i] : -HUGE_VAL, h = a.hi ? a.hi[prob * a.bstride + i] : HUGE_VAL;
      const bool lg = a.logmask >> i & 1;
      g[i] = a.grad[prob * k + i];
      ok = ok && cov_finite(g[i]) && cov_finite(th) && l <= th && th <= h && !(lg && th <= 0.0);
#pragma unroll
      for (int j = i; j < k; j++) ok = ok && cov_finite(A[i * NK + j][lane]);
      s[i] = lg ? th : 1.0;
      // (held needs theta and the bounds once: the mask is finished below, when gs is known)
      heldm |= (th <= l ? 1u : 0u) << i | (th >= h ? 1u : 0u) << (NK + i);
    }
#pragma unroll
    for (int i = 0; i < k; i++) {
      g[i] = s[i] * g[i];
      Hd[i] = (s[i] * s[i]) * A[i * NK + i][lane];
      ok = ok && cov_finite(g[i]) && cov_finite(Hd[i]) && !(Hd[i] < 0.0);
#pragma unroll
      for (int j = i + 1; j < k; j++) { const double v = (s[i] * s[j]) * A[i * NK + j][lane]; A[i * NK + j][lane] = v; ok = ok && cov_finite(v); }
    }
    unsigned hm = 0;
#pragma unroll
    for (int i = 0; i < k; i++) {
      const bool held = ((heldm >> i & 1) && g[i] > 0.0) || ((heldm >> (NK + i) & 1) && g[i] < 0.0);
      const bool unseen = !held && Hd[i] == 0.0;
      hm |= (held ? 1u : 0u) << i; unm |= (unseen ? 1u : 0u) << i;
      r[i] = (held || unseen) ? 1.0 : sqrt(Hd[i]);
    }
    heldm = hm; anm = ~(heldm | unm) & ((1u << k) - 1u);
    if (ok) {
      fm = (int)(~heldm & ((1u << k) - 1u));
      int n_free = 0;
#pragma unroll
      for (int i = 0; i < k; i++) { n_free += fm >> i & 1; n_an += (int)(anm >> i & 1); }
      if (unm) st |= PLH_COV_UNSEEN | (int)(unm << 8);
      if (n_an == 0) st |= PLH_COV_NO_FREE;
      sg2 = 1.0;
      if (a.n_data) {
        const int dof = a.n_data[prob] - n_free;
        if (dof <= 0) { sg2 = qnan; st |= PLH_COV_NO_DOF; }
        else sg2 = (2.0 * cost) / (double)dof;
      }
      // C over the analysed keys in A's strict upper triangle, an identity row for every other key
#pragma unroll
      for (int i = 0; i < k; i++)
#pragma unroll
        for (int j = i + 1; j < k; j++) A[i * NK + j][lane] = (anm >> i & anm >> j & 1) ? A[i * NK + j][lane] / (r[i] * r[j]) : 0.0;
      // C = L L^T row by row: L_ij (i > j) -> A[8 i + j], L_ii -> A[8 i + i]
#pragma unroll
      for (int i = 0; i < k; i++) {
#pragma unroll
        for (int j = 0; j < i; j++) {
          double v = A[j * NK + i][lane];
#pragma unroll
          for (int p = 0; p < j; p++) v -= A[i * NK + p][lane] * A[j * NK + p][lane];
          A[i * NK + j][lane] = v / A[j * NK + j][lane];
        }
        double v = 1.0;
#pragma unroll
        for (int p = 0; p < i; p++) v -= A[i * NK + p][lane] * A[i * NK + p][lane];
        if (!(v > 0.0) || !cov_finite(v)) { sing = true; v = 1.0; }
        A[i * NK + i][lane] = sqrt(v);
      }
      if (sing) st |= PLH_COV_SINGULAR;
      // X = L^-1 in place, column by column (column j reads L's columns >= j only, and its own entries above)
#pragma unroll
      for (int j = 0; j < k; j++) {
        A[j * NK + j][lane] = 1.0 / A[j * NK + j][lane];
#pragma unroll
        for (int i = j + 1; i < k; i++) {
          double v = A[i * NK + j][lane] * A[j * NK + j][lane];
#pragma unroll
          for (int p = j + 1; p < i; p++) v += A[i * NK + p][lane] * A[p * NK + j][lane];
          A[i * NK + j][lane] = -(v / A[i * NK + i][lane]);
        }
      }
      // P = X^T X in place, row by row: P_ij = sum over p >= i of X_pi X_pj  (j <= i; entry (i, j) reads rows >= i only)
#pragma unroll
      for (int i = 0; i < k; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
          double v = A[i * NK + i][lane] * A[i * NK + j][lane];
#pragma unroll
          for (int p = i + 1; p < k; p++) v += A[p * NK + i][lane] * A[p * NK + j][lane];
          A[i * NK + j][lane] = v;
        }
    }
    // cov -> B (both triangles), stderr
#pragma unroll
    for (int i = 0; i < k; i++)
#pragma unroll
      for (int j = 0; j <= i; j++) {
        double v = qnan;
        if (ok) {
          const double c = (s[i] * s[j]) * ((A[i * NK + j][lane] * sg2) / (r[i] * r[j]));
          v = ((heldm >> i | heldm >> j) & 1) ? 0.0 : ((unm >> i | unm >> j) & 1) ? qnan : sing ? qnan : c;
        }
        B[i * NK + j][lane] = v; B[j * NK + i][lane] = v;
        if (j == i) a.se[prob * k + i] = !ok ? qnan : (heldm >> i & 1) ? 0.0 : (unm >> i & 1) ? HUGE_VAL : sqrt(v);
      }
    a.sigma2[prob] = sg2; a.free_mask[prob] = fm;
  }
  __syncthreads();
  for (int x = lane; x < nb * kk; x += TILE) a.cov[p0 * kk + x] = B[ent(x % kk)][x / kk];
  __syncthreads();

  // corr -> B
  if (live) {
#pragma unroll
    for (int i = 0; i < k; i++)
#pragma unroll
      for (int j = 0; j <= i; j++) {
        double v = qnan;
        if (ok) {
          const double c = j == i ? 1.0 : A[i * NK + j][lane] / sqrt(A[i * NK + i][lane] * A[j * NK + j][lane]);
          v = ((heldm >> i | heldm >> j) & 1) ? 0.0 : ((unm >> i | unm >> j) & 1) ? qnan : sing ? qnan : c;
        }
        B[i * NK + j][lane] = v; B[j * NK + i][lane] = v;
      }
  }
  __syncthreads();
  for (int x = lane; x < nb * kk; x += TILE) a.corr[p0 * kk + x] = B[ent(x % kk)][x / kk];
  __syncthreads();

  // ---- the eigen-decomposition of C: cyclic Jacobi on A's upper triangle, V in B
  if (live) {
    double ev[K];
#pragma unroll
    for (int i = 0; i < k; i++) ev[i] = qnan;
    if (ok) {
#pragma unroll
      for (int i = 0; i < k; i++) {
        A[i * NK + i][lane] = 1.0;
#pragma unroll
        for (int j = 0; j < k; j++) B[i * NK + j][lane] = i == j ? 1.0 : 0.0;
      }
      bool rot = true;
      for (int sw = 0; sw < PLH_COV_MAX_SWEEPS && rot; sw++) {
        rot = false;
#pragma unroll
        for (int p = 0; p < k; p++)
#pragma unroll
          for (int q = p + 1; q < k; q++) {
            const double apq = A[p * NK + q][lane], app = A[p * NK + p][lane], aqq = A[q * NK + q][lane];
            if (fabs(apq) <= DBL_EPSILON * sqrt(fabs(app * aqq))) { A[p * NK + q][lane] = 0.0; continue; }
            rot = true;
            const double th = (aqq - app) / (2.0 * apq);
            const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c, tau = sn / (1.0 + c);
            A[p * NK + p][lane] = app - t * apq; A[q * NK + q][lane] = aqq + t * apq; A[p * NK + q][lane] = 0.0;
#pragma unroll
            for (int x = 0; x < k; x++) if (x != p && x != q) {
              const int ip = x < p ? x * NK + p : p * NK + x, iq = x < q ? x * NK + q : q * NK + x;
              const double g = A[ip][lane], h = A[iq][lane];
              A[ip][lane] = g - sn * (h + tau * g); A[iq][lane] = h + sn * (g - tau * h);
            }
#pragma unroll
            for (int x = 0; x < k; x++) {
              const double g = B[x * NK + p][lane], h = B[x * NK + q][lane];
              B[x * NK + p][lane] = g - sn * (h + tau * g); B[x * NK + q][lane] = h + sn * (g - tau * h);
            }
          }
      }
      if (rot) st |= PLH_COV_SWEEPS;
      // ascending, the keys that are not analysed last: conditional swaps of neighbouring columns (strict >: ties keep the Jacobi column order)
#pragma unroll
      for (int i = 0; i < k; i++) ev[i] = (anm >> i & 1) ? A[i * NK + i][lane] : HUGE_VAL;
#pragma unroll
      for (int pass = 0; pass < k - 1; pass++)
#pragma unroll
        for (int j = 0; j < k - 1 - pass; j++)
          if (ev[j] > ev[j + 1]) {
            const double e = ev[j]; ev[j] = ev[j + 1]; ev[j + 1] = e;
#pragma unroll
            for (int x = 0; x < k; x++) { const double v = B[x * NK + j][lane]; B[x * NK + j][lane] = B[x * NK + j + 1][lane]; B[x * NK + j + 1][lane] = v; }
          }
    }
    // the sign rule; rows >= n_an are NaN
#pragma unroll
    for (int j = 0; j < k; j++) {
      double big = -1.0, at = 0.0;
#pragma unroll
      for (int x = 0; x < k; x++) { const double v = B[x * NK + j][lane]; if (fabs(v) > big) { big = fabs(v); at = v; } }
      const bool given = ok && j < n_an;
      const double f = at < 0.0 ? -1.0 : 1.0;
#pragma unroll
      for (int x = 0; x < k; x++) B[x * NK + j][lane] = given ? f * B[x * NK + j][lane] : qnan;
      a.eval[prob * k + j] = given ? ev[j] : qnan;
    }
    a.coll[prob] = !ok || n_an == 0 ? qnan : ev[0] <= 0.0 ? HUGE_VAL : 1.0 / sqrt(ev[0]);
    a.status[prob] = ok ? st : PLH_COV_BAD_INPUT;
  }
  __syncthreads();
  // evec[j][i] = V_ij: the segment store reads B transposed
  for (int x = lane; x < nb * kk; x += TILE) { const int e = x % kk; a.evec[p0 * kk + x] = B[e % K * NK + e / K][x / kk]; }
}

inline void launch(hipStream_t st, const Args& a) {
  const unsigned grid = (unsigned)((a.n + TILE - 1) / TILE);
  switch (a.n_keys) {
    case 1: PL_LAUNCH(k_fit_cov<1>, grid, TILE, st, a); break;
    case 2: PL_LAUNCH(k_fit_cov<2>, grid, TILE, st, a); break;
    case 3: PL_LAUNCH(k_fit_cov<3>, grid, TILE, st, a); break;
    case 4: PL_LAUNCH(k_fit_cov<4>, grid, TILE, st, a); break;
    case 5: PL_LAUNCH(k_fit_cov<5>, grid, TILE, st, a); break;
    case 6: PL_LAUNCH(k_fit_cov<6>, grid, TILE, st, a); break;
    case 7: PL_LAUNCH(k_fit_cov<7>, grid, TILE, st, a); break;
    default: PL_LAUNCH(k_fit_cov<8>, grid, TILE, st, a); break;
  }
}

}  // namespace plcov

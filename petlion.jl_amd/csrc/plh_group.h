// plh_group.h -- parameters shared by groups of consecutive cells: plh_lsq_group (the fits of a group's members summed into one fit per group) and plh_group_scatter (the keys of
// a group's theta row copied to the rows of its members).  include/petlion_hip.h states the definition.  Like plh_resample.h / plh_lsq.h / plh_lm.h: no model variant, host
// translation unit.  A grouping is group_off[n_groups + 1] (ascending, 0 .. n_cells): group g owns the cells group_off[g] .. group_off[g + 1] - 1.
//
//   k_lsq_group      one block = one wave = one group, lanes = entries.  The k x k matrices are cell-major, so the JtJ of a group's members is ONE contiguous segment and the
//                    k^2 <= 64 entries of a member are one coalesced load of the wave; a second, short pass (k + 1 <= 9 lanes) takes grad and cost.  A lane sums ITS entry over
//                    the members sequentially, in ascending cell order, starting from the first member's value: only additions, nothing to contract, and no lane ever combines
//                    with another -- the bits are those of a plain loop on the host whatever the launch shape.  The sum is a chain of dependent adds behind loads: the loads of
//                    BATCH members are issued ahead of the adds that consume them, and the next batch is in flight while the current one is added (a group of 2 .. 10 members
//                    is one batch; one group of thousands is a chain of n / BATCH load latencies on one wave).  A member past the end is neither loaded nor added (the
//                    condition is the same in every lane): adding a zero instead would turn a sum of -0.0 into +0.0.
//                    The status of the group: lanes stride the members, one butterfly (0 / 1 in doubles: exact, any order gives the same maximum).
//   k_group_scatter  one block = one wave = one group, lanes = (member, key) pairs: theta[c][cols[i]] = g_theta[g][cols[i]].  Nothing else of theta is touched.
#pragma once

#include "plh_resample.h"

namespace plgr {

constexpr int NK = PLH_LSQ_MAX_SENS;      // keys at most
constexpr int TILE = 64;                  // lanes per block
constexpr int BATCH = 8;                  // members whose loads are issued together

struct SumArgs {
  int n_sens;
  const int* group_off;                                                       // [n_groups + 1], device
  const double* cost; const double* grad; const double* JtJ; const int* status;      // status may be NULL (0 everywhere)
  double* g_cost; double* g_grad; double* g_JtJ; int* g_status;                      // g_status may be NULL
};

// the sum of src[c * stride] over the members c0 <= c < c1, in ascending order from the first member's value (every lane of the wave calls it with the same c0, c1)
__device__ inline double sum_members(const double* src, size_t stride, long long c0, long long c1) {
  double acc = src[(size_t)c0 * stride];
  double cur[BATCH], nxt[BATCH];
#pragma unroll
  for (int j = 0; j < BATCH; j++) { cur[j] = 0.0; if (c0 + 1 + j < c1) cur[j] = src[(size_t)(c0 + 1 + j) * stride]; }
  for (long long c = c0 + 1; c < c1; c += BATCH) {
#pragma unroll
    for (int j = 0; j < BATCH; j++) { nxt[j] = 0.0; if (c + BATCH + j < c1) nxt[j] = src[(size_t)(c + BATCH + j) * stride]; }
#pragma unroll
    for (int j = 0; j < BATCH; j++) if (c + j < c1) acc += cur[j];
#pragma unroll
    for (int j = 0; j < BATCH; j++) cur[j] = nxt[j];
  }
  return acc;
}

__global__ void __launch_bounds__(TILE) k_lsq_group(SumArgs a) {
  const int lane = (int)threadIdx.x, g = (int)blockIdx.x;
  const int c0 = a.group_off[g], c1 = a.group_off[g + 1];
  const int k = a.n_sens, kk = k * k;
  // pass 1: lanes = the entries of JtJ
  if (lane < kk) a.g_JtJ[(size_t)g * kk + lane] = sum_members(a.JtJ + lane, (size_t)kk, c0, c1);
  // pass 2: lanes 0 .. k - 1 = grad, lane k = cost
  if (lane < k) a.g_grad[(size_t)g * k + lane] = sum_members(a.grad + lane, (size_t)k, c0, c1);
  else if (lane == k) a.g_cost[g] = sum_members(a.cost, 1, c0, c1);
  if (!a.g_status) return;                                            // (the same in every lane)
  double bad = 0.0;
  if (a.status) for (long long c = (long long)c0 + lane; c < c1; c += TILE) bad = fmax(bad, a.status[c] != 0 ? 1.0 : 0.0);
  for (int m = TILE / 2; m >= 1; m >>= 1) bad = fmax(bad, __shfl_xor(bad, m));
  if (lane == 0) a.g_status[g] = (int)bad;
}

struct ScatterArgs {
  int n_theta, n_keys;
  int cols[NK];
  const int* group_off;                                               // [n_groups + 1], device
  const double* g_theta; double* theta;
};

__global__ void __launch_bounds__(TILE) k_group_scatter(ScatterArgs a) {
  const int lane = (int)threadIdx.x, g = (int)blockIdx.x;
  const int c0 = a.group_off[g], c1 = a.group_off[g + 1];
  const size_t n = (size_t)(c1 - c0) * a.n_keys;
  for (size_t x = (size_t)lane; x < n; x += TILE) {
    const size_t c = (size_t)c0 + x / a.n_keys; const int col = a.cols[x % a.n_keys];
    a.theta[c * a.n_theta + col] = a.g_theta[(size_t)g * a.n_theta + col];
  }
}

inline void launch_sum(hipStream_t st, int n_groups, const SumArgs& a) { PL_LAUNCH(k_lsq_group, (unsigned)n_groups, TILE, st, a); }
inline void launch_scatter(hipStream_t st, int n_groups, const ScatterArgs& a) { PL_LAUNCH(k_group_scatter, (unsigned)n_groups, TILE, st, a); }

}  // namespace plgr

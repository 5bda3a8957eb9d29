// The "one wave per crystal" reduction of the per-crystal figures (eval_ops.hip, export_ops.hip, frame_ops.hip,
// series_ops.hip, and through bond_graph.h bond_ops.hip, bond_table_ops.hip, riding_ops.hip, molecule_ops.hip, tls_ops.hip
// and aniso_h_ops.hip): a workgroup of one wave owns crystal g, lane l takes rows l, l + 64, ... of the crystal in
// row order into fp64 accumulators, the 64 lane values are folded by a butterfly (o = 32, 16, ..., 1: the same pairs in the
// same order on every run) and lane 0 stores.  No atomics, fixed order: two runs give the same bytes.  Every kernel keeps
// its own per-row expression and its own store; what they share is the clamped row range and the folds.
#pragma once
#include "common.h"

#include <math.h>

// rows [r0, r1) of crystal g in the [B+1] offsets, clamped to an array of n rows
__device__ __forceinline__ void cr_rows(const int64_t* __restrict__ ptr, int g, int64_t n, int64_t& r0, int64_t& r1) {
  r0 = ptr[g];
  r1 = ptr[g + 1];
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > n ? n : r1;
}

// the maximum that keeps a NaN (fmax would drop it): the step of a running maximum and of its fold
__device__ __forceinline__ double cr_max_nan(double hi, double other) { return (other > hi || other != other) ? other : hi; }

// The folds over the 64 lanes; every lane returns the result.
__device__ __forceinline__ double cr_wave_sum(double s) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return s;
}

__device__ __forceinline__ double cr_wave_max_nan(double hi) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) hi = cr_max_nan(hi, __shfl_xor(hi, o));
  return hi;
}

__device__ __forceinline__ double cr_wave_min(double lo) {             // fmin: a NaN is dropped
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) lo = fmin(lo, __shfl_xor(lo, o));
  return lo;
}

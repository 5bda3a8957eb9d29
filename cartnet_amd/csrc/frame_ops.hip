// Mean of the predictions of one batch over K rotated frames.  CartNet in its default (non-invariant) mode reads cart_dir in
// the frame the crystal is stored in and is only approximately rotation-equivariant; the reference measures the gap
// (main.py:62-119: the input is cart_dir @ R, main.py:95, and an equivariant model would return R^T U R, main.py:97).
// cartnet_adp_frame_mean closes it for predictions: member k of a row, predicted from cart_dir @ R_k, is brought back to the
// stored frame as U_k = R_k P_k R_k^T, and the row gets the mean over the members and the largest deviation from it.
//
//   cn_frame_mean_kernel          per row, in fp64 from the fp32 inputs, k ascending, every product and sum in a fixed order
//                                 (explicit fma chains: the host and the device form of fm_frame_mean_row give the same
//                                 bits), results stored as fp32 with one rounding: mean = (1/K) sum_k U_k, spread = the
//                                 largest |U_k - mean| over members and components against the fp64 mean.  The members are
//                                 formed twice (sum, then deviations) so that K stays a run-time number without scratch.  A
//                                 row finds its crystal by the tile / binary-search scheme of shard_tiles.h, as
//                                 cn_adp_export_kernel (export_ops.hip) does.
//   cn_frame_mean_crystal_kernel  one wave per crystal: crystal_spread[g] = (sum, maximum) of the fp32 spread as stored
//                                 (crystal_reduce.h; the maximum keeps a NaN).
//   cn_stored_frame_kernel        cartnet_adp_stored_frame: the way back of a model that reads every crystal in ONE other frame
//                                 (iComformer in the frame of its reduced cell, dataset/datasetADP.py:75-80): out = R_g P R_g^T
//                                 by the same fm_member, one rotation per crystal shared by the T temperature slices of pred
//                                 (blockIdx.y), one launch, no mean and no spread.
//
// No symmetrisation (the export does its own), the rotations are used as given.  No atomics, fixed order: two runs give the
// same bytes.  Neither kernel uses scratch or LDS.
#include "common.h"
#include "crystal_reduce.h"
#include "shard_tiles.h"

#include <math.h>

namespace {

// U = R P R^T of one member: t = P R^T, then R t; each element a chain of two fma on the first product, in index order.
// With R the identity every chain is 1 * p + 0 + 0: U has P's values exactly.
__host__ __device__ __forceinline__ void fm_member(const float* __restrict__ p, const float* __restrict__ rf, double u[9]) {
  double P[9], R[9], t[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    P[q] = (double)p[q];
    R[q] = (double)rf[q];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      t[a * 3 + c] = fma(P[a * 3 + 2], R[c * 3 + 2], fma(P[a * 3 + 1], R[c * 3 + 1], P[a * 3] * R[c * 3]));
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      u[a * 3 + c] = fma(R[a * 3 + 2], t[6 + c], fma(R[a * 3 + 1], t[3 + c], R[a * 3] * t[c]));
}

// One row: pred = the row's 3x3 in frame 0, the other members pstride floats apart; rot = the frame-0 rotation of the row's
// crystal, the other frames rstride floats apart.  A NaN member makes mean and spread NaN.  Also compiled for the host, where
// a stand-alone program can check the arithmetic.
__host__ __device__ __forceinline__ void fm_frame_mean_row(const float* __restrict__ pred, int64_t pstride,
                                                           const float* __restrict__ rot, int64_t rstride, int K,
                                                           float* __restrict__ mean, float* __restrict__ spread) {
#pragma clang fp contract(off)
  double m[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, u[9];
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    fm_member(pred + k * pstride, rot + k * rstride, u);
#pragma unroll
    for (int q = 0; q < 9; ++q) m[q] += u[q];
  }
  const double n = (double)K;
#pragma unroll
  for (int q = 0; q < 9; ++q) m[q] = m[q] / n;
  double s = 0.0;
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    fm_member(pred + k * pstride, rot + k * rstride, u);
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      const double d = fabs(u[q] - m[q]);
      s = (d > s || d != d) ? d : s;                              // a NaN is kept, not dropped as fmax would
    }
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) mean[q] = (float)m[q];
  *spread = (float)s;
}

__global__ __launch_bounds__(SO_THREADS) void cn_frame_mean_kernel(const float* __restrict__ pred,
                                                                   const float* __restrict__ rot, int K,
                                                                   const int64_t* __restrict__ ptr, int B, int64_t M,
                                                                   float* __restrict__ mean, float* __restrict__ spread) {
  const int64_t t0 = (int64_t)blockIdx.x * SO_TILE, i0 = t0 + (int64_t)threadIdx.x * SO_ITEMS;
  if (i0 >= M) return;
  int g = so_walk_first(ptr, B, M, t0, i0);
#pragma unroll 1
  for (int k = 0; k < SO_ITEMS; ++k) {
    const int64_t i = i0 + k;
    if (i >= M) break;
    g = so_walk_to(ptr, B, g, i);                                 // steps over empty crystals
    fm_frame_mean_row(pred + i * 9, M * 9, rot + (size_t)g * 9, (int64_t)B * 9, K, mean + i * 9, spread + i);
  }
}

// One row of cartnet_adp_stored_frame: out = R P R^T, the member of fm_member stored with one rounding.  With R the identity
// out has pred's values exactly; a NaN in pred makes the row's results NaN and touches no other row.  Also compiled for the
// host, as fm_frame_mean_row is.
__host__ __device__ __forceinline__ void fm_stored_frame_row(const float* __restrict__ pred, const float* __restrict__ rot,
                                                             float* __restrict__ out) {
#pragma clang fp contract(off)
  double u[9];
  fm_member(pred, rot, u);
#pragma unroll
  for (int q = 0; q < 9; ++q) out[q] = (float)u[q];
}

// blockIdx.y = the temperature slice: its M rows share row_ptr and the B rotations with every other slice.
__global__ __launch_bounds__(SO_THREADS) void cn_stored_frame_kernel(const float* __restrict__ pred,
                                                                     const float* __restrict__ rot,
                                                                     const int64_t* __restrict__ ptr, int B, int64_t M,
                                                                     float* __restrict__ out) {
  const int64_t t0 = (int64_t)blockIdx.x * SO_TILE, i0 = t0 + (int64_t)threadIdx.x * SO_ITEMS;
  if (i0 >= M) return;
  const int64_t slice = (int64_t)blockIdx.y * M;
  int g = so_walk_first(ptr, B, M, t0, i0);
#pragma unroll 1
  for (int k = 0; k < SO_ITEMS; ++k) {
    const int64_t i = i0 + k;
    if (i >= M) break;
    g = so_walk_to(ptr, B, g, i);                                 // steps over empty crystals
    fm_stored_frame_row(pred + (slice + i) * 9, rot + (size_t)g * 9, out + (slice + i) * 9);
  }
}

__global__ __launch_bounds__(WAVE) void cn_frame_mean_crystal_kernel(const int64_t* __restrict__ ptr, int64_t M,
                                                                     const float* __restrict__ spread,
                                                                     double* __restrict__ stats) {
  const int g = blockIdx.x, lane = threadIdx.x;
  int64_t r0, r1;
  cr_rows(ptr, g, M, r0, r1);
  double sum = 0.0, hi = 0.0;
  for (int64_t r = r0 + lane; r < r1; r += WAVE) {
    const double s = (double)spread[r];
    sum += s;
    hi = cr_max_nan(hi, s);
  }
  sum = cr_wave_sum(sum);
  hi = cr_wave_max_nan(hi);
  if (lane == 0) {
    stats[(size_t)g * 2 + 0] = sum;
    stats[(size_t)g * 2 + 1] = hi;
  }
}

}  // namespace

extern "C" int cartnet_adp_frame_mean(const float* pred, const float* rot, int32_t K, const int64_t* row_ptr, int32_t B,
                                      int64_t M, float* mean, float* spread, double* crystal_spread, void* stream) {
  CN_CHECK(K >= 1 && B >= 0 && M >= 0, "cartnet_adp_frame_mean: bad sizes (K=%d, B=%d, M=%lld)", K, B, (long long)M);
  CN_CHECK(M < (1LL << 31) * SO_TILE / 4, "cartnet_adp_frame_mean: too many rows for one launch");
  if (M == 0 || B == 0) return 0;
  CN_CHECK(pred && rot && row_ptr && mean && spread, "cartnet_adp_frame_mean: null pointer");
  CN_CHECK(mean != pred && spread != pred && (const void*)crystal_spread != (const void*)pred,
           "cartnet_adp_frame_mean: an output must not alias pred");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cn_frame_mean_kernel, dim3((unsigned)((M + SO_TILE - 1) / SO_TILE)), dim3(SO_THREADS), 0, st, pred,
                     rot, K, row_ptr, B, M, mean, spread);
  CN_LAUNCH_CHECK("cartnet_adp_frame_mean");
  if (crystal_spread) {
    hipLaunchKernelGGL(cn_frame_mean_crystal_kernel, dim3(B), dim3(WAVE), 0, st, row_ptr, M, spread, crystal_spread);
    CN_LAUNCH_CHECK("cartnet_adp_frame_mean");
  }
  return 0;
}

extern "C" int cartnet_adp_stored_frame(const float* pred, const float* rotation, const int64_t* row_ptr, int32_t B,
                                        int64_t M, int32_t T, float* out, void* stream) {
  CN_CHECK(T >= 1 && T <= 65535 && B >= 0 && M >= 0, "cartnet_adp_stored_frame: bad sizes (T=%d, B=%d, M=%lld)", T, B,
           (long long)M);
  CN_CHECK(M < (1LL << 31) * SO_TILE / 4, "cartnet_adp_stored_frame: too many rows for one launch");
  if (M == 0 || B == 0) return 0;
  CN_CHECK(pred && rotation && row_ptr && out, "cartnet_adp_stored_frame: null pointer");
  CN_CHECK(out != pred, "cartnet_adp_stored_frame: out must not alias pred");
  hipLaunchKernelGGL(cn_stored_frame_kernel, dim3((unsigned)((M + SO_TILE - 1) / SO_TILE), (unsigned)T), dim3(SO_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), pred, rotation, row_ptr, B, M, out);
  CN_LAUNCH_CHECK("cartnet_adp_stored_frame");
  return 0;
}

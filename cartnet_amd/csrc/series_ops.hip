// A least-squares line per row and component through the exported ADPs of one batch over T temperatures.  The node encoder
// takes the temperature in (cartnet_node_embed: emb[z] + the temperature projection), so one checkpoint answers "what do the
// ellipsoids look like at 100 K, 150 K, ... 300 K"; the reference predicts at the one temperature a crystal is stored with
// (main.py:21-60).  ADPs must grow with T, roughly linearly above the zero-point regime: cartnet_adp_temp_series turns the T
// exports of a row into the line's slope and intercept, the largest residual and the number of steps on which U_eq falls.
//
//   cn_temp_series_kernel          per row, in fp64 from the fp32 inputs, t ascending, contraction off, every result stored
//                                  as fp32 with one rounding; seven columns (c = 0..5 of u_cif, c = 6 = u_eq):
//                                    tbar = (sum_t T_t) / T, Stt = sum_t (T_t - tbar)^2
//                                    centre_c = (sum_t u_tc) / T, slope_c = (sum_t (T_t - tbar) u_tc) / Stt
//                                    intercept_c = centre_c - slope_c tbar                (the line at 0 K)
//                                    resid = the largest |u_tc - (centre_c + slope_c (T_t - tbar))| over t and c, NaN kept
//                                    drops = the number of t with u_eq[t+1] < u_eq[t]
//                                  The members are read twice (sums, then residuals) so that T stays a run-time number
//                                  without scratch.  A row needs no crystal; the tiling is shard_tiles.h's (SO_TILE rows per
//                                  workgroup, SO_ITEMS consecutive rows per thread), as cn_frame_mean_kernel's (frame_ops.hip).
//   cn_temp_series_crystal_kernel  one wave per crystal (crystal_reduce.h), from the values as stored: the sum of the U_eq
//                                  slopes, the rows whose U_eq slope is not > 0 (a NaN counts), the rows with drops > 0, the
//                                  maximum of resid (NaN kept).
//
// No atomics, fixed order: two runs give the same bytes.  Neither kernel uses scratch or LDS.
#include "common.h"
#include "crystal_reduce.h"
#include "shard_tiles.h"

#include <math.h>

namespace {

constexpr int TS_COLS = 7;                                          // U11 U22 U33 U23 U13 U12 of u_cif, then u_eq

// tbar and Stt of the T temperatures: the same for every row, taken once per thread.
__host__ __device__ __forceinline__ void ts_moments(const float* __restrict__ temps, int T, double& tbar, double& stt) {
#pragma clang fp contract(off)
  double s = 0.0;
#pragma unroll 1
  for (int t = 0; t < T; ++t) s += (double)temps[t];
  tbar = s / (double)T;
  stt = 0.0;
#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    const double d = (double)temps[t] - tbar;
    stt += d * d;
  }
}

// One row: cif = the row's six values at the first temperature, the other members cstride floats apart; eq = its u_eq at the
// first temperature, the others estride floats apart.  A NaN member makes slope, intercept (of its column) and resid NaN.
// Also compiled for the host, where a stand-alone program can check the arithmetic.
__host__ __device__ __forceinline__ void ts_series_row(const float* __restrict__ cif, int64_t cstride,
                                                       const float* __restrict__ eq, int64_t estride,
                                                       const float* __restrict__ temps, int T, double tbar, double stt,
                                                       float* __restrict__ slope, float* __restrict__ intercept,
                                                       float* __restrict__ resid, int32_t* __restrict__ drops) {
#pragma clang fp contract(off)
  double su[TS_COLS], sx[TS_COLS];
#pragma unroll
  for (int c = 0; c < TS_COLS; ++c) su[c] = sx[c] = 0.0;
  int32_t nd = 0;
  float prev = 0.f;
#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    const double d = (double)temps[t] - tbar;
    const float* __restrict__ p = cif + t * cstride;
    const float e = eq[t * estride];
#pragma unroll
    for (int c = 0; c < TS_COLS; ++c) {
      const double u = (double)(c < 6 ? p[c] : e);
      su[c] += u;
      sx[c] += d * u;
    }
    nd += (t > 0 && e < prev) ? 1 : 0;                            // strict; a NaN on either side is no drop
    prev = e;
  }
  const double n = (double)T;
  double ce[TS_COLS], sl[TS_COLS];
#pragma unroll
  for (int c = 0; c < TS_COLS; ++c) {
    ce[c] = su[c] / n;
    sl[c] = sx[c] / stt;
  }
  double r = 0.0;
#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    const double d = (double)temps[t] - tbar;
    const float* __restrict__ p = cif + t * cstride;
    const float e = eq[t * estride];
#pragma unroll
    for (int c = 0; c < TS_COLS; ++c) {
      const double u = (double)(c < 6 ? p[c] : e);
      const double a = fabs(u - (ce[c] + sl[c] * d));
      r = (a > r || a != a) ? a : r;                              // a NaN is kept, not dropped as fmax would
    }
  }
#pragma unroll
  for (int c = 0; c < TS_COLS; ++c) {
    slope[c] = (float)sl[c];
    intercept[c] = (float)(ce[c] - sl[c] * tbar);
  }
  *resid = (float)r;
  *drops = nd;
}

__global__ __launch_bounds__(SO_THREADS) void cn_temp_series_kernel(const float* __restrict__ u_cif,
                                                                    const float* __restrict__ u_eq,
                                                                    const float* __restrict__ temps, int T, int64_t M,
                                                                    float* __restrict__ slope, float* __restrict__ intercept,
                                                                    float* __restrict__ resid, int32_t* __restrict__ drops) {
  const int64_t i0 = (int64_t)blockIdx.x * SO_TILE + (int64_t)threadIdx.x * SO_ITEMS;
  if (i0 >= M) return;
  double tbar, stt;
  ts_moments(temps, T, tbar, stt);
#pragma unroll 1
  for (int k = 0; k < SO_ITEMS; ++k) {
    const int64_t i = i0 + k;
    if (i >= M) break;
    ts_series_row(u_cif + i * 6, M * 6, u_eq + i, M, temps, T, tbar, stt, slope + i * TS_COLS, intercept + i * TS_COLS,
                  resid + i, drops + i);
  }
}

__global__ __launch_bounds__(WAVE) void cn_temp_series_crystal_kernel(const int64_t* __restrict__ ptr, int64_t M,
                                                                      const float* __restrict__ slope,
                                                                      const float* __restrict__ resid,
                                                                      const int32_t* __restrict__ drops,
                                                                      double* __restrict__ stats) {
  const int g = blockIdx.x, lane = threadIdx.x;
  int64_t r0, r1;
  cr_rows(ptr, g, M, r0, r1);
  double sum = 0.0, flat = 0.0, fell = 0.0, hi = 0.0;
  for (int64_t r = r0 + lane; r < r1; r += WAVE) {
    const float s = slope[r * TS_COLS + 6];
    sum += (double)s;
    flat += (s > 0.f) ? 0.0 : 1.0;                                // not > 0: a NaN counts
    fell += (drops[r] > 0) ? 1.0 : 0.0;
    hi = cr_max_nan(hi, (double)resid[r]);
  }
  sum = cr_wave_sum(sum);
  flat = cr_wave_sum(flat);
  fell = cr_wave_sum(fell);
  hi = cr_wave_max_nan(hi);
  if (lane == 0) {
    stats[(size_t)g * 4 + 0] = sum;
    stats[(size_t)g * 4 + 1] = flat;
    stats[(size_t)g * 4 + 2] = fell;
    stats[(size_t)g * 4 + 3] = hi;
  }
}

}  // namespace

extern "C" int cartnet_adp_temp_series(const float* u_cif, const float* u_eq, const float* temps, int32_t T,
                                       const int64_t* row_ptr, int32_t B, int64_t M, float* slope, float* intercept,
                                       float* resid, int32_t* drops, double* crystal_stats, void* stream) {
  CN_CHECK(T >= 2 && B >= 0 && M >= 0, "cartnet_adp_temp_series: bad sizes (T=%d, B=%d, M=%lld)", T, B, (long long)M);
  CN_CHECK(M < (1LL << 31) * SO_TILE / 4, "cartnet_adp_temp_series: too many rows for one launch");
  if (M == 0 || B == 0) return 0;
  CN_CHECK(u_cif && u_eq && temps && row_ptr && slope && intercept && resid && drops,
           "cartnet_adp_temp_series: null pointer");
  const void* const ins[3] = {u_cif, u_eq, temps};
  const void* const outs[5] = {slope, intercept, resid, drops, crystal_stats};
  for (const void* o : outs)
    for (const void* in : ins)
      CN_CHECK(o != in, "cartnet_adp_temp_series: an output must not alias an input");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cn_temp_series_kernel, dim3((unsigned)((M + SO_TILE - 1) / SO_TILE)), dim3(SO_THREADS), 0, st, u_cif,
                     u_eq, temps, T, M, slope, intercept, resid, drops);
  CN_LAUNCH_CHECK("cartnet_adp_temp_series");
  if (crystal_stats) {
    hipLaunchKernelGGL(cn_temp_series_crystal_kernel, dim3(B), dim3(WAVE), 0, st, row_ptr, M, slope, resid, drops,
                       crystal_stats);
    CN_LAUNCH_CHECK("cartnet_adp_temp_series");
  }
  return 0;
}

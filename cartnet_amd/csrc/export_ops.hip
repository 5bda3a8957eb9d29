// Export of predicted ADPs in the convention crystallographic tools read.  The dataset's targets were brought into the
// Cartesian frame by the reference's dataset/extract_csd_data.py:115-123: U_cart = A (N U_cif N) A^T with A = cell^T
// (columns a, b, c) and N = diag(|a*|, |b*|, |c*|).  cartnet_adp_export goes the other way: the rows of inv(A) are the
// reciprocal vectors a*_i, so U_cif[i][j] = (a*_i / |a*_i|)^T U_cart (a*_j / |a*_j|) = r^_i^T U r^_j.
//
//   cn_adp_export_kernel   per row, in fp64 from the fp32 inputs, results stored as fp32: U = (U + U^T) / 2, U_cif, U_eq =
//                          tr(U) / 3, and the principal values / axes of U by a cyclic Jacobi iteration with a fixed number
//                          of sweeps (no trigonometric closed form: it loses the small value of a flat ellipsoid), sorted
//                          ascending, each axis with its largest component positive.  A row finds its crystal by the tile /
//                          binary-search scheme of shard_tiles.h, as cn_rotate_rows_kernel (eval_ops.hip) does.
//   cn_adp_export_crystal_kernel  one wave per crystal: status[g] (bit 0: singular cell) and crystal_stats[g] = (sum of
//                          U_eq, smallest principal value, rows whose smallest principal value <= 0) from the fp32 values as
//                          stored (crystal_reduce.h).
//
// No atomics, fixed order: two runs give the same bytes.  Neither kernel uses scratch or LDS.
#include "common.h"
#include "crystal_reduce.h"
#include "shard_tiles.h"

#include <math.h>

namespace {

constexpr int EX_SWEEPS = 8;   // a 3x3 cyclic Jacobi converges quadratically: 5 sweeps reach fp64 round-off, 8 leave a margin

// The unit reciprocal vectors r[i][.] of the cell whose rows are the lattice vectors a, b, c (fp32): a* = (b x c) / det,
// b* = (c x a) / det, c* = (a x b) / det with det = a . (b x c); only their directions are needed, so each cross product is
// normalised on its own and takes det's sign.  False if det == 0 or it is not finite (r is then NaN).
__host__ __device__ __forceinline__ bool ex_reciprocal_units(const float* __restrict__ cell, double r[3][3]) {
  double a[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) a[i][j] = (double)cell[i * 3 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int p = (i + 1) % 3, q = (i + 2) % 3;
    r[i][0] = a[p][1] * a[q][2] - a[p][2] * a[q][1];
    r[i][1] = a[p][2] * a[q][0] - a[p][0] * a[q][2];
    r[i][2] = a[p][0] * a[q][1] - a[p][1] * a[q][0];
  }
  const double det = a[0][0] * r[0][0] + a[0][1] * r[0][1] + a[0][2] * r[0][2];
  const bool ok = det != 0.0 && isfinite(det);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double n = sqrt(r[i][0] * r[i][0] + r[i][1] * r[i][1] + r[i][2] * r[i][2]);
    const double s = ok ? (det < 0.0 ? -1.0 : 1.0) / n : (double)NAN;
#pragma unroll
    for (int j = 0; j < 3; ++j) r[i][j] = ok ? r[i][j] * s : (double)NAN;
  }
  return ok;
}

// One Jacobi rotation in the (p, q) plane, o the third index (all three compile-time constants after inlining): the
// symmetric matrix is held as d[3] (diagonal) and the off-diagonal elements e_pq, e_po, e_qo; the eigenvector estimates
// are the COLUMNS of v.
__host__ __device__ __forceinline__ void ex_jacobi_rotate(double& dp, double& dq, double& e_pq, double& e_po,
                                                          double& e_qo, double v[3][3], const int p, const int q) {
  if (e_pq == 0.0) return;
  const double theta = (dq - dp) / (2.0 * e_pq);
  const double at = fabs(theta);
  // the smaller root of t^2 + 2 t theta - 1 = 0; theta^2 would overflow far beyond 1e100, where t = 1 / (2 theta) exactly
  double t = at > 1e100 ? 0.5 / at : 1.0 / (at + sqrt(theta * theta + 1.0));
  t = theta < 0.0 ? -t : t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  dp -= t * e_pq;
  dq += t * e_pq;
  e_pq = 0.0;
  const double po = c * e_po - s * e_qo, qo = s * e_po + c * e_qo;
  e_po = po;
  e_qo = qo;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = c * v[k][p] - s * v[k][q], vq = s * v[k][p] + c * v[k][q];
    v[k][p] = vp;
    v[k][q] = vq;
  }
}

__host__ __device__ __forceinline__ void ex_swap_cols(double d[3], double v[3][3], const int i, const int j) {
  if (d[j] < d[i]) {
    const double t = d[i]; d[i] = d[j]; d[j] = t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double w = v[k][i]; v[k][i] = v[k][j]; v[k][j] = w;
    }
  }
}

// One row: up = the 3x3 fp32 input, r = the crystal's unit reciprocal vectors (NaN for a singular cell: every output of
// the row is then NaN).  Also compiled for the host, where a stand-alone program can check the arithmetic.
__host__ __device__ __forceinline__ void ex_export_row(const float* __restrict__ up, const double r[3][3],
                                                       float* __restrict__ cif, float* __restrict__ ueq,
                                                       float* __restrict__ prin, float* __restrict__ axes) {
  const bool ok = r[0][0] == r[0][0];
  double u[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) u[a][b] = 0.5 * ((double)up[a * 3 + b] + (double)up[b * 3 + a]);
  // U_cif = r^ U r^T: w = U r^_j, then r^_i . w; order U11 U22 U33 U23 U13 U12
  double w[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int a = 0; a < 3; ++a) w[j][a] = u[a][0] * r[j][0] + u[a][1] * r[j][1] + u[a][2] * r[j][2];
  const int ci[6] = {0, 1, 2, 1, 0, 0}, cj[6] = {0, 1, 2, 2, 2, 1};
#pragma unroll
  for (int q = 0; q < 6; ++q)
    cif[q] = (float)(r[ci[q]][0] * w[cj[q]][0] + r[ci[q]][1] * w[cj[q]][1] + r[ci[q]][2] * w[cj[q]][2]);
  const double nanv = (double)NAN;
  *ueq = (float)(ok ? (u[0][0] + u[1][1] + u[2][2]) / 3.0 : nanv);
  double d[3] = {u[0][0], u[1][1], u[2][2]};
  double e01 = u[0][1], e02 = u[0][2], e12 = u[1][2];
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll 1
  for (int sweep = 0; sweep < EX_SWEEPS; ++sweep) {
    ex_jacobi_rotate(d[0], d[1], e01, e02, e12, v, 0, 1);         // (p, q) = (0, 1): e_po = e02, e_qo = e12
    ex_jacobi_rotate(d[0], d[2], e02, e01, e12, v, 0, 2);         // (0, 2): e_po = e01, e_qo = e21
    ex_jacobi_rotate(d[1], d[2], e12, e01, e02, v, 1, 2);         // (1, 2): e_po = e10, e_qo = e20
  }
  ex_swap_cols(d, v, 0, 1);
  ex_swap_cols(d, v, 1, 2);
  ex_swap_cols(d, v, 0, 1);
#pragma unroll
  for (int c = 0; c < 3; ++c) prin[c] = (float)(ok ? d[c] : nanv);
  if (axes) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {                                 // axis c = column c of v; its largest component positive
      const double x = v[0][c], y = v[1][c], z = v[2][c];
      const double ax = fabs(x), ay = fabs(y), az = fabs(z);
      const double big = ax >= ay && ax >= az ? x : (ay >= az ? y : z);
      const double sg = ok ? (big < 0.0 ? -1.0 : 1.0) : nanv;
      axes[c * 3 + 0] = (float)(x * sg);
      axes[c * 3 + 1] = (float)(y * sg);
      axes[c * 3 + 2] = (float)(z * sg);
    }
  }
}

__global__ __launch_bounds__(SO_THREADS) void cn_adp_export_kernel(const float* __restrict__ u_cart,
                                                                   const int64_t* __restrict__ ptr,
                                                                   const float* __restrict__ cell, int B, int64_t M,
                                                                   float* __restrict__ u_cif, float* __restrict__ u_eq,
                                                                   float* __restrict__ principal,
                                                                   float* __restrict__ axes) {
  const int64_t t0 = (int64_t)blockIdx.x * SO_TILE, i0 = t0 + (int64_t)threadIdx.x * SO_ITEMS;
  if (i0 >= M) return;
  int g = so_walk_first(ptr, B, M, t0, i0);
  int loaded = -1;
  double r[3][3];
#pragma unroll 1
  for (int k = 0; k < SO_ITEMS; ++k) {
    const int64_t i = i0 + k;
    if (i >= M) break;
    g = so_walk_to(ptr, B, g, i);                                 // steps over empty crystals
    if (g != loaded) {
      ex_reciprocal_units(cell + (size_t)g * 9, r);                // NaN for a singular cell: its rows come out NaN
      loaded = g;
    }
    ex_export_row(u_cart + i * 9, r, u_cif + i * 6, u_eq + i, principal + i * 3, axes ? axes + i * 9 : nullptr);
  }
}

__global__ __launch_bounds__(WAVE) void cn_adp_export_crystal_kernel(const int64_t* __restrict__ ptr,
                                                                     const float* __restrict__ cell, int64_t M,
                                                                     const float* __restrict__ u_eq,
                                                                     const float* __restrict__ principal,
                                                                     double* __restrict__ stats,
                                                                     int32_t* __restrict__ status) {
  const int g = blockIdx.x, lane = threadIdx.x;
  if (lane == 0) {
    double r[3][3];
    status[g] = ex_reciprocal_units(cell + (size_t)g * 9, r) ? 0 : 1;
  }
  if (!stats) return;
  int64_t r0, r1;
  cr_rows(ptr, g, M, r0, r1);
  double sum = 0.0, lo = (double)INFINITY, bad = 0.0;
  for (int64_t r = r0 + lane; r < r1; r += WAVE) {
    const double p = (double)principal[r * 3];
    sum += (double)u_eq[r];
    lo = fmin(lo, p);
    bad += p <= 0.0 ? 1.0 : 0.0;
  }
  sum = cr_wave_sum(sum);
  lo = cr_wave_min(lo);
  bad = cr_wave_sum(bad);
  if (lane == 0) {
    stats[(size_t)g * 3 + 0] = sum;
    stats[(size_t)g * 3 + 1] = lo;
    stats[(size_t)g * 3 + 2] = bad;
  }
}

}  // namespace

extern "C" int cartnet_adp_export(const float* u_cart, const int64_t* row_ptr, const float* cell, int32_t B, int64_t M,
                                  float* u_cif, float* u_eq, float* principal, float* axes, double* crystal_stats,
                                  int32_t* status, void* stream) {
  CN_CHECK(B >= 0 && M >= 0, "cartnet_adp_export: bad sizes (B=%d, M=%lld)", B, (long long)M);
  CN_CHECK(M < (1LL << 31) * SO_TILE / 4, "cartnet_adp_export: too many rows for one launch");
  if (M == 0 || B == 0) return 0;
  CN_CHECK(u_cart && row_ptr && cell && u_cif && u_eq && principal && status, "cartnet_adp_export: null pointer");
  CN_CHECK(u_cif != u_cart && u_eq != u_cart && principal != u_cart && axes != u_cart,
           "cartnet_adp_export: an output must not alias u_cart");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cn_adp_export_kernel, dim3((unsigned)((M + SO_TILE - 1) / SO_TILE)), dim3(SO_THREADS), 0, st, u_cart,
                     row_ptr, cell, B, M, u_cif, u_eq, principal, axes);
  CN_LAUNCH_CHECK("cartnet_adp_export");
  hipLaunchKernelGGL(cn_adp_export_crystal_kernel, dim3(B), dim3(WAVE), 0, st, row_ptr, cell, M, u_eq, principal,
                     crystal_stats, status);
  CN_LAUNCH_CHECK("cartnet_adp_export");
  return 0;
}

// Hirshfeld's rigid-bond test on predicted ADPs (Hirshfeld, Acta Cryst. A32 (1976) 239; the PLAT23x alerts of checkCIF): for
// two covalently bonded atoms the mean-square displacement amplitudes along the bond are nearly equal,
// D = d^T U_i d - d^T U_j d ~ 0.  The reference has no counterpart: its only statements about a prediction need the truth
// (main.py:47-49).  The test needs none; it reads the batch's radius graph, whose edges hold the periodic images solved
// (cart_dir, cart_dist) and are sorted by target atom.
//
// A directed edge e = (j -> i) is a bond by the rule of bond_graph.h (bg_bond), with every atom of the batch admissible as
// a source; the group layout, the ordered fold and the quadratic form are that header's too.
//
//   cn_bond_test_kernel          BG_LANES lanes per atom: they stride the atom's edge segment, sixteen edges a pass, and
//                                filter on cart_dist and z[source] first; only a bond gathers its direction and the
//                                partner's nine floats.  Per bond, in fp64 from the fp32 inputs,
//                                D = d^T (S_i - S_j) d with S = (U + U^T) / 2 (the difference is taken first), d as
//                                stored.  The bonds of a pass are then folded in EDGE order (bg_walk, bg_fold): the sum is
//                                the sequential fp64 sum over the edges, and a tie of |D| keeps the lowest edge.
//   cn_bond_test_crystal_kernel  one wave per crystal: bg_pair_stats over the rows' bonds.
//
// No atomics, no workgroup waits for another, fixed order: two runs give the same bytes.  64-bit offsets throughout.
// Neither kernel uses scratch or LDS.
#include "bond_graph.h"

namespace {

// d^T (S_i - S_j) d, and the trace of U_j
__device__ __forceinline__ double bt_delta(const double ui[9], const float* __restrict__ uj, const float* __restrict__ dir,
                                           double& trace_j) {
  double w[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) w[q] = (double)uj[q];
  trace_j = w[0] + w[4] + w[8];
#pragma unroll
  for (int q = 0; q < 9; ++q) w[q] = ui[q] - w[q];
  return bg_form(w, (double)dir[0], (double)dir[1], (double)dir[2]);
}

__global__ __launch_bounds__(BG_THREADS) void cn_bond_test_kernel(
    const float* __restrict__ u, const int64_t* __restrict__ z, const int64_t* __restrict__ src,
    const float* __restrict__ cart_dist, const float* __restrict__ cart_dir, const int64_t* __restrict__ atom_row,
    const int64_t* __restrict__ seg_ptr, const float* __restrict__ radii, int n_radii, float tol, double threshold,
    int64_t N, int64_t M, int64_t E, int32_t* __restrict__ bonds, float* __restrict__ delta_sum,
    float* __restrict__ delta_max, int64_t* __restrict__ worst, int32_t* __restrict__ over,
    float* __restrict__ ueq_ratio) {
  const BondGraph g = {z, src, cart_dist, atom_row, seg_ptr, radii, n_radii, tol, N, M, E};
  const int lane = threadIdx.x & (WAVE - 1), sub = lane & (BG_LANES - 1), base = lane - sub;
  const int64_t i = (int64_t)blockIdx.x * BG_ATOMS + (threadIdx.x / BG_LANES);
  int64_t m = -1, zi = 0, e0 = 0, e1 = 0;
  if (i < N) m = bg_row(atom_row, i, M);                           // -1: nothing to write
  if (m >= 0) {
    zi = z[i];
    bg_segment(seg_ptr, i, E, e0, e1);
    if (zi <= 1 || zi >= n_radii) e1 = e0;                        // hydrogen, 0 or beyond the table: never bonded
  }
  double ui[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  float ri = 0.f;
  if (e1 > e0) {
    ri = radii[zi];
#pragma unroll
    for (int q = 0; q < 9; ++q) ui[q] = (double)u[m * 9 + q];
  }
  BgFold f;
  double traces = 0.0;
#pragma unroll 1
  for (int64_t c = e0; c < e1; c += BG_LANES) {
    const int64_t e = c + sub;
    int64_t j = -1, mj = -1;
    double a = 0.0, tj = 0.0;
    const bool bond = e < e1 && bg_bond(g, i, ri, e, 0, N, j, mj);
    if (bond) a = fabs(bt_delta(ui, u + mj * 9, cart_dir + e * 3, tj));
    bg_walk(bond, base, [&](int l) {                               // the bonds of this pass, lowest edge first
      bg_fold(f, __shfl(a, l), __shfl((long long)j, l), threshold);
      traces += __shfl(tj, l);
    });
  }
  if (m >= 0 && sub == 0) {
    bonds[m] = f.n;
    delta_sum[m] = (float)f.sum;
    delta_max[m] = (float)f.hi;
    worst[m] = f.who;
    over[m] = f.over;
    ueq_ratio[m] = f.n ? (float)((ui[0] + ui[4] + ui[8]) / (traces / (double)f.n)) : NAN;
  }
}

__global__ __launch_bounds__(WAVE) void cn_bond_test_crystal_kernel(const int64_t* __restrict__ row_ptr, int64_t M,
                                                                    const int32_t* __restrict__ bonds,
                                                                    const float* __restrict__ delta_sum,
                                                                    const float* __restrict__ delta_max,
                                                                    const int32_t* __restrict__ over,
                                                                    double* __restrict__ stats) {
  bg_pair_stats(row_ptr, M, bonds, delta_sum, delta_max, over, stats);
}

}  // namespace

extern "C" int cartnet_adp_bond_test(const float* u, const int64_t* z, const int64_t* edge_index, const float* cart_dist,
                                     const float* cart_dir, const int64_t* atom_row, const int64_t* seg_ptr,
                                     const int64_t* row_ptr, const float* radii, int32_t n_radii, float tol,
                                     double threshold, int32_t B, int64_t N, int64_t M, int64_t E, int32_t* bonds,
                                     float* delta_sum, float* delta_max, int64_t* worst, int32_t* over, float* ueq_ratio,
                                     double* crystal_stats, void* stream) {
  CN_CHECK(B >= 0 && N >= 0 && M >= 0 && E >= 0 && n_radii >= 0,
           "cartnet_adp_bond_test: bad sizes (B=%d, N=%lld, M=%lld, E=%lld, n_radii=%d)", B, (long long)N, (long long)M,
           (long long)E, n_radii);
  CN_CHECK(tol == tol && threshold == threshold, "cartnet_adp_bond_test: tol and threshold must be numbers");
  CN_CHECK(N < (1LL << 31) * BG_ATOMS, "cartnet_adp_bond_test: too many atoms for one launch");
  if (M == 0 || B == 0 || N == 0) return 0;
  CN_CHECK(u && z && atom_row && seg_ptr && row_ptr && bonds && delta_sum && delta_max && worst && over && ueq_ratio,
           "cartnet_adp_bond_test: null pointer");
  CN_CHECK(E == 0 || (edge_index && cart_dist && cart_dir && radii), "cartnet_adp_bond_test: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // without edges every segment is empty: the rows get their neutral values from the same launch
  hipLaunchKernelGGL(cn_bond_test_kernel, dim3((unsigned)((N + BG_ATOMS - 1) / BG_ATOMS)), dim3(BG_THREADS), 0, st, u, z,
                     edge_index, cart_dist, cart_dir, atom_row, seg_ptr, radii, (int)n_radii, tol, threshold, N, M, E,
                     bonds, delta_sum, delta_max, worst, over, ueq_ratio);
  CN_LAUNCH_CHECK("cartnet_adp_bond_test");
  if (crystal_stats) {
    hipLaunchKernelGGL(cn_bond_test_crystal_kernel, dim3(B), dim3(WAVE), 0, st, row_ptr, M, bonds, delta_sum, delta_max,
                       over, crystal_stats);
    CN_LAUNCH_CHECK("cartnet_adp_bond_test");
  }
  return 0;
}

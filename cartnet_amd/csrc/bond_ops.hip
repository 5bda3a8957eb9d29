// Hirshfeld's rigid-bond test on predicted ADPs (Hirshfeld, Acta Cryst. A32 (1976) 239; the PLAT23x alerts of checkCIF): for
// two covalently bonded atoms the mean-square displacement amplitudes along the bond are nearly equal,
// D = d^T U_i d - d^T U_j d ~ 0.  The reference has no counterpart: its only statements about a prediction need the truth
// (main.py:47-49).  The test needs none; it reads the batch's radius graph, whose edges hold the periodic images solved
// (cart_dir, cart_dist) and are sorted by target atom.
//
// A directed edge e = (j -> i) is a bond when i != j, both atomic numbers are non-hydrogen and inside the radii table, and
// cart_dist[e] <= (r[z_i] + r[z_j]) + tol in fp32 in exactly that order (additions only: numpy fp32 gives the same bits).
//
//   cn_bond_test_kernel          BT_LANES lanes per atom: they stride the atom's edge segment, sixteen edges a pass, and
//                                filter on cart_dist and z[source] first; only a bond gathers its direction and the
//                                partner's nine floats.  Per bond, in fp64 from the fp32 inputs,
//                                D = d^T (S_i - S_j) d with S = (U + U^T) / 2 (the difference is taken first: it is exact
//                                for fp32 inputs of like size, so the cancellation costs nothing), d as stored.  The bonds of
//                                a pass are then folded in EDGE order: the group's slice of the wave's ballot names them,
//                                and every lane of the group reads them one by one with a shuffle from the named lane.  So
//                                the sum is the sequential fp64 sum over the edges, and a tie of |D| keeps the lowest edge.
//   cn_bond_test_crystal_kernel  one wave per crystal: crystal_stats[g] = (sum of bonds, sum of delta_sum, maximum of
//                                delta_max, sum of over) of the values as stored (crystal_reduce.h; the maximum keeps a
//                                NaN).
//
// No atomics, no workgroup waits for another, fixed order: two runs give the same bytes.  64-bit offsets throughout.
// Neither kernel uses scratch or LDS.
#include "common.h"
#include "crystal_reduce.h"

#include <math.h>

namespace {

constexpr int BT_LANES = 16;                     // lanes per atom: an atom has ~100 incoming edges at radius 5
constexpr int BT_THREADS = 256;
constexpr int BT_ATOMS = BT_THREADS / BT_LANES;  // atoms per workgroup

// d^T (S_i - S_j) d with S the symmetric part: the off-diagonal pairs enter as (u_ab + u_ba), which is 2 S_ab exactly.
__device__ __forceinline__ double bt_delta(const double ui[9], const float* __restrict__ uj, const float* __restrict__ dir,
                                           double& trace_j) {
  double w[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) w[q] = (double)uj[q];
  trace_j = w[0] + w[4] + w[8];
#pragma unroll
  for (int q = 0; q < 9; ++q) w[q] = ui[q] - w[q];
  const double x = (double)dir[0], y = (double)dir[1], z = (double)dir[2];
  return w[0] * x * x + w[4] * y * y + w[8] * z * z + (w[1] + w[3]) * x * y + (w[2] + w[6]) * x * z + (w[5] + w[7]) * y * z;
}

__global__ __launch_bounds__(BT_THREADS) void cn_bond_test_kernel(
    const float* __restrict__ u, const int64_t* __restrict__ z, const int64_t* __restrict__ src,
    const float* __restrict__ cart_dist, const float* __restrict__ cart_dir, const int64_t* __restrict__ atom_row,
    const int64_t* __restrict__ seg_ptr, const float* __restrict__ radii, int n_radii, float tol, double threshold,
    int64_t N, int64_t M, int64_t E, int32_t* __restrict__ bonds, float* __restrict__ delta_sum,
    float* __restrict__ delta_max, int64_t* __restrict__ worst, int32_t* __restrict__ over,
    float* __restrict__ ueq_ratio) {
  const int lane = threadIdx.x & (WAVE - 1), sub = lane & (BT_LANES - 1), base = lane - sub;
  const int64_t i = (int64_t)blockIdx.x * BT_ATOMS + (threadIdx.x / BT_LANES);
  // every lane of a group takes the same branch below: a group is never split, and a shuffle reads its own group only
  int64_t m = -1, zi = 0, e0 = 0, e1 = 0;
  if (i < N) {
    m = atom_row[i];
    if (m < 0 || m >= M) m = -1;                                  // a hydrogen (or an index that is no row): nothing to write
  }
  if (m >= 0) {
    zi = z[i];
    e0 = seg_ptr[i];
    e1 = seg_ptr[i + 1];
    e0 = e0 < 0 ? 0 : (e0 > E ? E : e0);
    e1 = e1 < e0 ? e0 : (e1 > E ? E : e1);
    if (zi <= 1 || zi >= n_radii) e1 = e0;                        // hydrogen, 0 or beyond the table: never bonded
  }
  double ui[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  float ri = 0.f;
  if (e1 > e0) {
    ri = radii[zi];
#pragma unroll
    for (int q = 0; q < 9; ++q) ui[q] = (double)u[m * 9 + q];
  }
  int32_t n_bonds = 0, n_over = 0;
  double sum = 0.0, hi = 0.0, traces = 0.0;
  int64_t who = -1;
#pragma unroll 1
  for (int64_t c = e0; c < e1; c += BT_LANES) {
    const int64_t e = c + sub;
    bool bond = false;
    int64_t j = -1;
    double a = 0.0, tj = 0.0;
    if (e < e1) {
      const float dist = cart_dist[e];
      j = src[e];
      if (j != i && j >= 0 && j < N) {
        const int64_t zj = z[j];
        if (zj > 1 && zj < n_radii) {
          const float limit = (ri + radii[zj]) + tol;
          const int64_t mj = atom_row[j];
          if (dist <= limit && mj >= 0 && mj < M) {
            bond = true;
            a = fabs(bt_delta(ui, u + mj * 9, cart_dir + e * 3, tj));
          }
        }
      }
    }
    unsigned int found = (unsigned int)((__ballot(bond) >> base) & ((1ull << BT_LANES) - 1));
    while (found) {                                                // the bonds of this pass, lowest edge first
      const int l = base + __builtin_ctz(found);
      found &= found - 1;
      const double av = __shfl(a, l), tv = __shfl(tj, l);
      const long long jv = __shfl((long long)j, l);
      n_bonds += 1;
      sum += av;
      traces += tv;
      n_over += av > threshold ? 1 : 0;
      if (av > hi || who < 0 || (av != av && hi == hi)) {         // a tie keeps the earlier edge; a NaN is kept
        hi = av;
        who = jv;
      }
    }
  }
  if (m >= 0 && sub == 0) {
    bonds[m] = n_bonds;
    delta_sum[m] = (float)sum;
    delta_max[m] = (float)hi;
    worst[m] = who;
    over[m] = n_over;
    ueq_ratio[m] = n_bonds ? (float)((ui[0] + ui[4] + ui[8]) / (traces / (double)n_bonds)) : NAN;
  }
}

__global__ __launch_bounds__(WAVE) void cn_bond_test_crystal_kernel(const int64_t* __restrict__ ptr, int64_t M,
                                                                    const int32_t* __restrict__ bonds,
                                                                    const float* __restrict__ delta_sum,
                                                                    const float* __restrict__ delta_max,
                                                                    const int32_t* __restrict__ over,
                                                                    double* __restrict__ stats) {
  const int g = blockIdx.x, lane = threadIdx.x;
  int64_t r0, r1;
  cr_rows(ptr, g, M, r0, r1);
  double nb = 0.0, sum = 0.0, hi = 0.0, no = 0.0;
  for (int64_t r = r0 + lane; r < r1; r += WAVE) {
    const double s = (double)delta_max[r];
    nb += (double)bonds[r];
    sum += (double)delta_sum[r];
    hi = cr_max_nan(hi, s);
    no += (double)over[r];
  }
  nb = cr_wave_sum(nb);
  sum = cr_wave_sum(sum);
  hi = cr_wave_max_nan(hi);
  no = cr_wave_sum(no);
  if (lane == 0) {
    stats[(size_t)g * 4 + 0] = nb;
    stats[(size_t)g * 4 + 1] = sum;
    stats[(size_t)g * 4 + 2] = hi;
    stats[(size_t)g * 4 + 3] = no;
  }
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
  CN_CHECK(N < (1LL << 31) * BT_ATOMS, "cartnet_adp_bond_test: too many atoms for one launch");
  if (M == 0 || B == 0 || N == 0) return 0;
  CN_CHECK(u && z && atom_row && seg_ptr && row_ptr && bonds && delta_sum && delta_max && worst && over && ueq_ratio,
           "cartnet_adp_bond_test: null pointer");
  CN_CHECK(E == 0 || (edge_index && cart_dist && cart_dir && radii), "cartnet_adp_bond_test: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // without edges every segment is empty: the rows get their neutral values from the same launch
  hipLaunchKernelGGL(cn_bond_test_kernel, dim3((unsigned)((N + BT_ATOMS - 1) / BT_ATOMS)), dim3(BT_THREADS), 0, st, u, z,
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

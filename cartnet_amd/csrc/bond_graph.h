// The bond graph of a batch on the device: what bond_ops.hip, bond_table_ops.hip, angle_table_ops.hip, riding_ops.hip,
// molecule_ops.hip, tls_ops.hip and aniso_h_ops.hip share, each rule written once.  The graph is the batch's radius graph
// (edges sorted by target atom, the periodic images solved in cart_dist / cart_dir) with the two lookups
// metrics.batch_graph builds: atom_row [N] (an atom's row in the model's output, -1 for a hydrogen) and seg_ptr [N+1] (atom
// i owns the edges [seg_ptr[i], seg_ptr[i+1])).  The rules are stated in cartnet_amd/bonds.py, which restates every kernel
// in numpy, bit for bit.
//
// Everything here is __device__ __forceinline__ and takes the compile flags of the file that includes it: aniso_h_ops.hip
// and angle_table_ops.hip are compiled with -ffp-contract=off, the others are not, and each keeps the contraction it had.
// bg_form is the only helper with products to contract; neither of the two calls it.
#pragma once
#include "common.h"
#include "crystal_reduce.h"

#include <math.h>

// ---- the group: BG_LANES lanes per atom (an atom has ~100 incoming edges at radius 5), BG_ATOMS atoms per workgroup.
// Lane `sub` of a group takes items c + sub of a pass.  A wave holds four whole groups and every lane of a group takes the
// same branches: a group is never split, and a shuffle reads its own group only.
constexpr int BG_LANES = 16;
constexpr int BG_THREADS = 256;
constexpr int BG_ATOMS = BG_THREADS / BG_LANES;

// the row of atom i, or -1 (a hydrogen, or an index that is no row)
__device__ __forceinline__ int64_t bg_row(const int64_t* __restrict__ atom_row, int64_t i, int64_t M) {
  const int64_t m = atom_row[i];
  return (m < 0 || m >= M) ? -1 : m;
}

// the edge segment of atom i, clamped to [0, E] and never negative in length
__device__ __forceinline__ void bg_segment(const int64_t* __restrict__ seg_ptr, int64_t i, int64_t E, int64_t& e0,
                                           int64_t& e1) {
  e0 = seg_ptr[i];
  e1 = seg_ptr[i + 1];
  e0 = e0 < 0 ? 0 : (e0 > E ? E : e0);
  e1 = e1 < e0 ? e0 : (e1 > E ? E : e1);
}

struct BondGraph {
  const int64_t* __restrict__ z;
  const int64_t* __restrict__ src;
  const float* __restrict__ cart_dist;
  const int64_t* __restrict__ atom_row;
  const int64_t* __restrict__ seg_ptr;
  const float* __restrict__ radii;
  int n_radii;
  float tol;
  int64_t N, M, E;
};

// The largest bonded distance of two atoms with covalent radii ri and rj: fp32, the radii first, then the tolerance --
// additions only and in exactly this order, so numpy fp32 gives the same bits (bonds.is_bond).
__device__ __forceinline__ float bg_limit(float ri, float rj, float tol) { return (ri + rj) + tol; }

// the same for a hydrogen and an atom of atomic number zp (1 < zp < n_radii): the riding rule's H bond
__device__ __forceinline__ float bg_h_limit(const BondGraph& g, int64_t zp) { return bg_limit(g.radii[1], g.radii[zp], g.tol); }

// Whether edge e = (j -> i) into atom i (covalent radius ri) is a bond; its source j and the source's row mj.  The caller
// has checked i's end (its atomic number, its row); here j is no image of i, lies in the admissible range [lo, hi) -- the
// batch, or i's crystal --, is no hydrogen and inside the radii table, is near enough (false for a NaN distance) and has
// a row, looked up last.
__device__ __forceinline__ bool bg_bond(const BondGraph& g, int64_t i, float ri, int64_t e, int64_t lo, int64_t hi,
                                        int64_t& j, int64_t& mj) {
  const float dist = g.cart_dist[e];
  j = g.src[e];
  if (j == i || j < lo || j >= hi) return false;
  const int64_t zj = g.z[j];
  if (zj <= 1 || zj >= g.n_radii) return false;
  if (!(dist <= bg_limit(ri, g.radii[zj], g.tol))) return false;
  mj = bg_row(g.atom_row, j, g.M);
  return mj >= 0;
}

// ---- the ordered fold: the items a group found in one pass, folded in ITEM order whatever lane holds them, so a sum is
// the sequential fp64 sum and a tie keeps the earlier item.  bg_walk calls step(l) with the wave lane l of every item of
// the group at `base` whose lane raised `flag`, lowest lane first; step reads the item with __shfl(value, l).
// the flags of the group at `base` alone, lane `sub` of the group in bit `sub`: a lane's rank among the raised flags is
// the population count of the bits below its own (angle_table_ops.hip; bond_table_ops.hip keeps its own copy, bt_flags)
__device__ __forceinline__ unsigned int bg_flags(bool flag, int base) {
  return (unsigned int)((__ballot(flag) >> base) & ((1ull << BG_LANES) - 1));
}

template <typename Step>
__device__ __forceinline__ void bg_walk(bool flag, int base, Step&& step) {
  unsigned int found = (unsigned int)((__ballot(flag) >> base) & ((1ull << BG_LANES) - 1));
  while (found) {
    step(base + __builtin_ctz(found));
    found &= found - 1;
  }
}

// the figures of a row over its items (bonds, or pairs of a molecule): their number, the sum and the maximum of |D|, the
// partner of the maximum, and how many lie over the threshold
struct BgFold {
  int32_t n = 0, over = 0;
  double sum = 0.0, hi = 0.0;
  int64_t who = -1;
};

__device__ __forceinline__ void bg_fold(BgFold& f, double a, int64_t partner, double threshold) {
  f.n += 1;
  f.sum += a;
  f.over += a > threshold ? 1 : 0;
  if (a > f.hi || f.who < 0 || (a != a && f.hi == f.hi)) {          // a tie keeps the earlier item; a NaN is kept
    f.hi = a;
    f.who = partner;
  }
}

// ---- the (dist, edge) minimum of a group: every lane brings the minimum over its own edges (at == E: none) and leaves
// with the group's, compared lexicographically (smaller dist, then the lower edge) -- the sequential minimum whatever the
// lane layout.
__device__ __forceinline__ void bg_argmin(float& best, int64_t& at, int64_t E) {
#pragma unroll
  for (int o = BG_LANES / 2; o > 0; o >>= 1) {
    const float d = __shfl_xor(best, o);
    const long long a = __shfl_xor((long long)at, o);
    if (a < E && (at == E || d < best || (d == best && a < at))) {
      best = d;
      at = a;
    }
  }
}

// v^T Sym(W) v for a row-major 3x3 W: the off-diagonal pairs enter as (w_ab + w_ba), which is 2 Sym(W)_ab exactly.  W is
// a difference U_i - U_j taken first: exact in fp64 for fp32 entries of like size, so the cancellation costs nothing.
__device__ __forceinline__ double bg_form(const double w[9], double x, double y, double z) {
  return w[0] * x * x + w[4] * y * y + w[8] * z * z + (w[1] + w[3]) * x * y + (w[2] + w[6]) * x * z + (w[5] + w[7]) * y * z;
}

// ---- the per-crystal figures of a pair statistic, one wave per crystal (crystal_reduce.h), of the values as stored:
// stats[g] = (sum of count, sum of delta_sum, maximum of delta_max -- it keeps a NaN --, sum of over)
__device__ __forceinline__ void bg_pair_stats(const int64_t* __restrict__ row_ptr, int64_t M,
                                              const int32_t* __restrict__ count, const float* __restrict__ delta_sum,
                                              const float* __restrict__ delta_max, const int32_t* __restrict__ over,
                                              double* __restrict__ stats) {
  const int g = blockIdx.x, lane = threadIdx.x;
  int64_t r0, r1;
  cr_rows(row_ptr, g, M, r0, r1);
  double n = 0.0, sum = 0.0, hi = 0.0, no = 0.0;
  for (int64_t r = r0 + lane; r < r1; r += WAVE) {
    n += (double)count[r];
    sum += (double)delta_sum[r];
    hi = cr_max_nan(hi, (double)delta_max[r]);
    no += (double)over[r];
  }
  n = cr_wave_sum(n);
  sum = cr_wave_sum(sum);
  hi = cr_wave_max_nan(hi);
  no = cr_wave_sum(no);
  if (lane == 0) {
    stats[(size_t)g * 4 + 0] = n;
    stats[(size_t)g * 4 + 1] = sum;
    stats[(size_t)g * 4 + 2] = hi;
    stats[(size_t)g * 4 + 3] = no;
  }
}

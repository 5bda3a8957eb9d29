// Riding hydrogens: an isotropic U for every hydrogen from the predicted U_eq of the atom it is bonded to (the riding model
// of crystallographic refinement; SHELXL's convention is 1.5 for methyl, hydroxyl and water hydrogens and 1.2 for all
// others).  The reference has no counterpart: its dataset keeps only the rows of non_H_mask (dataset/datasetADP.py:49), so a
// hydrogen never gets a displacement parameter.  This reads the batch's bond graph (bond_graph.h: the group layout, the
// segments and rows, the bond rule and the argmin of a group are that header's).
//
// An edge with a hydrogen at one end and the atom p at the other is an H bond when it is a bond by bg_bond with the
// hydrogen's radius at the hydrogen's end: 1 < z_p < n_radii, p has a row and cart_dist[e] <= bg_h_limit(z_p).  A NaN
// distance never qualifies.  The rule is stated in cartnet_amd/bonds.py (riding_hydrogens_host restates it in numpy).
//
//   cn_riding_parent_kernel   BG_LANES lanes per atom.  A hydrogen's group strides its edge segment, sixteen edges a pass,
//                             and filters on cart_dist and z[source] first; only then is the source's row looked up.  Each
//                             lane keeps its running (dist, edge) minimum; the group folds the pairs with bg_argmin.  Lane
//                             0 of the group writes parent[i] (-1: an orphan, or no hydrogen).
//   cn_riding_value_kernel    after the parent kernel on the same stream.  The group of atom i strides the segment of
//                             t = i (a non-hydrogen atom) or t = parent[i] (a hydrogen) and counts the edges s -> t with
//                             z[s] == 1, parent[s] == t and an H bond: integers, so the butterfly sum has no order.  A
//                             non-hydrogen atom stores the count and its own u_eq; a hydrogen takes n = max(count, 1),
//                             the multiplier (f_rot for z_t == 8, or z_t == 6 with n >= 3; f otherwise) and
//                             u_iso = fp32(fp64(mult) * fp64(u_eq[row of t])): exact product, one rounding.
//   cn_riding_crystal_kernel  one wave per crystal over its atoms: crystal_stats[g] = (hydrogens, orphans, sum of the
//                             finite hydrogen u_iso, hydrogens whose parent's u_eq is not positive), the crystal's atoms
//                             taking the place of rows in crystal_reduce.h.
//
// No atomics, no workgroup waits for another, fixed order: two runs give the same bytes.  64-bit offsets throughout.  No
// kernel uses scratch or LDS.
#include "bond_graph.h"

namespace {

__global__ __launch_bounds__(BG_THREADS) void cn_riding_parent_kernel(
    const int64_t* __restrict__ z, const int64_t* __restrict__ src, const float* __restrict__ cart_dist,
    const int64_t* __restrict__ atom_row, const int64_t* __restrict__ seg_ptr, const float* __restrict__ radii,
    int n_radii, float tol, int64_t N, int64_t M, int64_t E, int64_t* __restrict__ parent) {
  const BondGraph g = {z, src, cart_dist, atom_row, seg_ptr, radii, n_radii, tol, N, M, E};
  const int sub = threadIdx.x & (BG_LANES - 1);
  const int64_t i = (int64_t)blockIdx.x * BG_ATOMS + (threadIdx.x / BG_LANES);
  int64_t e0 = 0, e1 = 0;
  if (i < N && z[i] == 1) bg_segment(seg_ptr, i, E, e0, e1);
  const float rh = e1 > e0 && n_radii > 1 ? radii[1] : 0.f;
  float best = INFINITY;
  int64_t at = E;                                                  // E: no edge yet
#pragma unroll 1
  for (int64_t c = e0; c < e1; c += BG_LANES) {
    const int64_t e = c + sub;
    int64_t j, mj;
    if (e < e1 && bg_bond(g, i, rh, e, 0, N, j, mj)) {
      const float dist = cart_dist[e];
      if (dist < best || at == E) {                                // a lane's edges ascend: a tie keeps the earlier
        best = dist;
        at = e;
      }
    }
  }
  bg_argmin(best, at, E);
  if (i < N && sub == 0) {
    int64_t p = -1;
    if (at < E) p = src[at];
    parent[i] = p;
  }
}

__global__ __launch_bounds__(BG_THREADS) void cn_riding_value_kernel(
    const float* __restrict__ u_eq, const int64_t* __restrict__ z, const int64_t* __restrict__ src,
    const float* __restrict__ cart_dist, const int64_t* __restrict__ atom_row, const int64_t* __restrict__ seg_ptr,
    const float* __restrict__ radii, int n_radii, float tol, float f, float f_rot, int64_t N, int64_t M, int64_t E,
    const int64_t* __restrict__ parent, int32_t* __restrict__ count, float* __restrict__ mult,
    float* __restrict__ u_iso) {
  const BondGraph g = {z, src, cart_dist, atom_row, seg_ptr, radii, n_radii, tol, N, M, E};
  const int sub = threadIdx.x & (BG_LANES - 1);
  const int64_t i = (int64_t)blockIdx.x * BG_ATOMS + (threadIdx.x / BG_LANES);
  bool hydrogen = false;
  int64_t t = -1, zt = 0, e0 = 0, e1 = 0;
  if (i < N) {
    hydrogen = z[i] == 1;
    t = hydrogen ? parent[i] : i;
    if (t < 0 || t >= N) t = -1;
  }
  if (t >= 0) {
    zt = z[t];
    if (zt > 1 && zt < n_radii) bg_segment(seg_ptr, t, E, e0, e1);
  }
  const float limit = e1 > e0 ? bg_h_limit(g, zt) : 0.f;
  int32_t n = 0;
#pragma unroll 1
  for (int64_t c = e0; c < e1; c += BG_LANES) {
    const int64_t e = c + sub;
    if (e < e1 && cart_dist[e] <= limit) {
      const int64_t s = src[e];
      if (s >= 0 && s < N && z[s] == 1 && parent[s] == t) n += 1;
    }
  }
#pragma unroll
  for (int o = BG_LANES / 2; o > 0; o >>= 1) n += __shfl_xor(n, o);
  if (i < N && sub == 0) {
    const int64_t m = t >= 0 ? bg_row(atom_row, t, M) : -1;
    float k = 0.f, v = NAN;
    if (!hydrogen) {
      if (m >= 0) v = u_eq[m];
    } else if (m >= 0) {                                           // a parent always has a row
      const int32_t riders = n > 1 ? n : 1;
      k = (zt == 8 || (zt == 6 && riders >= 3)) ? f_rot : f;
      v = (float)((double)k * (double)u_eq[m]);
    }
    count[i] = hydrogen ? 0 : n;
    mult[i] = k;
    u_iso[i] = v;
  }
}

__global__ __launch_bounds__(WAVE) void cn_riding_crystal_kernel(const int64_t* __restrict__ atom_ptr, int64_t N, int64_t M,
                                                                 const float* __restrict__ u_eq,
                                                                 const int64_t* __restrict__ z,
                                                                 const int64_t* __restrict__ atom_row,
                                                                 const int64_t* __restrict__ parent,
                                                                 const float* __restrict__ u_iso,
                                                                 double* __restrict__ stats) {
  const int g = blockIdx.x, lane = threadIdx.x;
  int64_t a0, a1;
  cr_rows(atom_ptr, g, N, a0, a1);
  double nh = 0.0, orphans = 0.0, sum = 0.0, bad = 0.0;
  for (int64_t a = a0 + lane; a < a1; a += WAVE) {
    if (z[a] != 1) continue;
    nh += 1.0;
    const int64_t p = parent[a];
    const int64_t m = p >= 0 && p < N ? bg_row(atom_row, p, M) : -1;
    if (m < 0) {
      orphans += 1.0;
      continue;
    }
    const float v = u_iso[a];
    if (v - v == 0.f) sum += (double)v;                           // finite
    if (!(u_eq[m] > 0.f)) bad += 1.0;                             // not positive, or NaN
  }
  nh = cr_wave_sum(nh);
  orphans = cr_wave_sum(orphans);
  sum = cr_wave_sum(sum);
  bad = cr_wave_sum(bad);
  if (lane == 0) {
    stats[(size_t)g * 4 + 0] = nh;
    stats[(size_t)g * 4 + 1] = orphans;
    stats[(size_t)g * 4 + 2] = sum;
    stats[(size_t)g * 4 + 3] = bad;
  }
}

}  // namespace

extern "C" int cartnet_adp_riding_h(const float* u_eq, const int64_t* z, const int64_t* edge_index, const float* cart_dist,
                                    const int64_t* atom_row, const int64_t* seg_ptr, const int64_t* atom_ptr,
                                    const float* radii, int32_t n_radii, float tol, float f, float f_rot, int32_t B, int64_t N,
                                    int64_t M, int64_t E, int64_t* parent, int32_t* count, float* mult, float* u_iso,
                                    double* crystal_stats, void* stream) {
  CN_CHECK(B >= 0 && N >= 0 && M >= 0 && E >= 0 && n_radii >= 0,
           "cartnet_adp_riding_h: bad sizes (B=%d, N=%lld, M=%lld, E=%lld, n_radii=%d)", B, (long long)N, (long long)M,
           (long long)E, n_radii);
  CN_CHECK(tol == tol && f == f && f_rot == f_rot, "cartnet_adp_riding_h: tol, f and f_rot must be numbers");
  CN_CHECK(N < (1LL << 31) * BG_ATOMS, "cartnet_adp_riding_h: too many atoms for one launch");
  if (B == 0 || N == 0) return 0;
  CN_CHECK(z && atom_row && seg_ptr && parent && count && mult && u_iso, "cartnet_adp_riding_h: null pointer");
  CN_CHECK(M == 0 || u_eq, "cartnet_adp_riding_h: null pointer");
  CN_CHECK(E == 0 || (edge_index && cart_dist && radii), "cartnet_adp_riding_h: null pointer");
  CN_CHECK(!crystal_stats || atom_ptr, "cartnet_adp_riding_h: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((N + BG_ATOMS - 1) / BG_ATOMS));
  // without edges every segment is empty, without rows no atom is a parent: the same launches write the neutral values
  hipLaunchKernelGGL(cn_riding_parent_kernel, grid, dim3(BG_THREADS), 0, st, z, edge_index, cart_dist, atom_row, seg_ptr,
                     radii, (int)n_radii, tol, N, M, E, parent);
  CN_LAUNCH_CHECK("cartnet_adp_riding_h");
  hipLaunchKernelGGL(cn_riding_value_kernel, grid, dim3(BG_THREADS), 0, st, u_eq, z, edge_index, cart_dist, atom_row,
                     seg_ptr, radii, (int)n_radii, tol, f, f_rot, N, M, E, parent, count, mult, u_iso);
  CN_LAUNCH_CHECK("cartnet_adp_riding_h");
  if (crystal_stats) {
    hipLaunchKernelGGL(cn_riding_crystal_kernel, dim3(B), dim3(WAVE), 0, st, atom_ptr, N, M, u_eq, z, atom_row, parent,
                       u_iso, crystal_stats);
    CN_LAUNCH_CHECK("cartnet_adp_riding_h");
  }
  return 0;
}

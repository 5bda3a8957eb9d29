// Anisotropic hydrogens: a full displacement tensor for every hydrogen from three things the pass already has -- its
// parent's predicted tensor, the rigid-body motion of the parent's molecule (cartnet_adp_tls_fit) carried from the parent's
// position to the hydrogen's, and a nominal internal X-H motion in the bond frame.  This is the decomposition of SHADE
// (Madsen, J. Appl. Cryst. 39 (2006) 757) and of ADPH (Roversi & Destro, Chem. Phys. Lett. 386 (2004) 472).  The reference
// has no counterpart: a hydrogen never gets a displacement parameter there (dataset/datasetADP.py:49).  The rule is stated
// in cartnet_amd/bonds.py (aniso_hydrogens_host restates it in numpy).
//
//   cn_aniso_h_kernel          BG_LANES lanes per atom, the group layout of bond_graph.h.  The group of a hydrogen with a
//                              parent p strides the hydrogen's edge segment, sixteen edges a pass, and keeps per lane the
//                              running (dist, edge) minimum over the edges p -> i; the group folds the pairs with
//                              bg_argmin: the edge the riding rule chose.
//                              Lane 0 of the group then does the 3x3 arithmetic in fp64: v = dist * dir, d = v / |v|,
//                              Sym(U_p) + [U_LS(r_p + v) - U_LS(r_p)] + stretch d d^T + bend (I - d d^T), the six
//                              components of the upper triangle, each rounded once to fp32 and stored on both sides of the
//                              diagonal.  A non-hydrogen atom's lane 0 copies its own row bit for bit.
//   cn_aniso_h_crystal_kernel  one wave per crystal over its atoms, from the values as stored: crystal_stats[g] = (hydrogens
//                              with a tensor, those with source >= 3, the sum of their trace / 3, those whose tensor is not
//                              positive definite), the crystal's atoms taking the place of rows in crystal_reduce.h.
//
// This file is compiled with -ffp-contract=off: no multiply-add is fused, so |v|^2 and the minors of the crystal kernel are
// the numpy rule's operation for operation, and their decisions (> 0) fall alike; the helpers of bond_graph.h used here
// hold no product.  No atomics, no workgroup waits for another, fixed order: two runs give the same bytes.
// 64-bit offsets throughout.  No kernel uses scratch or LDS.
#include "bond_graph.h"

namespace {

// the six components 00 01 02 11 12 22 of U_LS(r) = A L A^T + A S + S^T A^T, A = [[0, z, -y], [-z, 0, x], [y, -x, 0]];
// L symmetric as 11 22 33 23 13 12, S row-major
__device__ __forceinline__ void ah_rigid(const double r[3], const double l6[6], const double s[9], double out[6]) {
  const double A[3][3] = {{0.0, r[2], -r[1]}, {-r[2], 0.0, r[0]}, {r[1], -r[0], 0.0}};
  const double L[3][3] = {{l6[0], l6[5], l6[4]}, {l6[5], l6[1], l6[3]}, {l6[4], l6[3], l6[2]}};
  double AL[3][3], AS[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      AL[a][b] = (A[a][0] * L[0][b] + A[a][1] * L[1][b]) + A[a][2] * L[2][b];
      AS[a][b] = (A[a][0] * s[0 + b] + A[a][1] * s[3 + b]) + A[a][2] * s[6 + b];
    }
  int k = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) {
      const double ala = (AL[a][0] * A[b][0] + AL[a][1] * A[b][1]) + AL[a][2] * A[b][2];
      out[k++] = ala + (AS[a][b] + AS[b][a]);
    }
}

__global__ __launch_bounds__(BG_THREADS) void cn_aniso_h_kernel(
    const float* __restrict__ u, const int64_t* __restrict__ z, const int64_t* __restrict__ src,
    const float* __restrict__ cart_dist, const float* __restrict__ cart_dir, const int64_t* __restrict__ atom_row,
    const int64_t* __restrict__ seg_ptr, const int64_t* __restrict__ parent, const double* __restrict__ x,
    const float* __restrict__ params, const int32_t* __restrict__ rank, double stretch, double bend, int64_t N, int64_t M,
    int64_t E, float* __restrict__ u_h, int32_t* __restrict__ source) {
  const int sub = threadIdx.x & (BG_LANES - 1);
  const int64_t i = (int64_t)blockIdx.x * BG_ATOMS + (threadIdx.x / BG_LANES);
  bool hydrogen = false;
  int64_t p = -1, mp = -1, e0 = 0, e1 = 0;
  if (i < N) {
    hydrogen = z[i] == 1;
    if (hydrogen) {
      p = parent[i];
      if (p < 0 || p >= N) p = -1;
      if (p >= 0) {
        mp = bg_row(atom_row, p, M);
        if (mp < 0) p = -1;
      }
    }
  }
  if (p >= 0) bg_segment(seg_ptr, i, E, e0, e1);
  float best = INFINITY;
  int64_t at = E;                                                  // E: no edge yet
#pragma unroll 1
  for (int64_t c = e0; c < e1; c += BG_LANES) {
    const int64_t e = c + sub;
    if (e < e1 && src[e] == p) {
      const float dist = cart_dist[e];
      if (dist < best) {                                           // a lane's edges ascend: a tie keeps the earlier
        best = dist;
        at = e;
      }
    }
  }
  bg_argmin(best, at, E);
  if (i >= N || sub != 0) return;
  float* __restrict__ out = u_h + (size_t)i * 9;
  int32_t code = 0;
  if (!hydrogen) {
    const int64_t m = bg_row(atom_row, i, M);
    if (m >= 0) {
      const float* __restrict__ row = u + (size_t)m * 9;
#pragma unroll
      for (int k = 0; k < 9; ++k) out[k] = row[k];
      source[i] = 1;
      return;
    }
  } else if (at < E) {
    const double len = (double)cart_dist[at];
    double v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = len * (double)cart_dir[(size_t)at * 3 + k];
    const double n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (n2 > 0.0) {                                                // false for a NaN
      const double n = sqrt(n2);
      const double d[3] = {v[0] / n, v[1] / n, v[2] / n};
      const float* __restrict__ row = u + (size_t)mp * 9;
      double lib[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      code = 2;
      const int32_t rk = (x && params && rank) ? rank[mp] : 0;
      if (rk > 0) {
        const float* __restrict__ pm = params + (size_t)mp * 24;
        double l6[6], s[9], rp[3], rh[3], at_p[6], at_h[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) l6[k] = (double)pm[6 + k];
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] = (double)pm[12 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          rp[k] = x[(size_t)p * 3 + k] - (double)pm[21 + k];
          rh[k] = rp[k] + v[k];
        }
        ah_rigid(rp, l6, s, at_p);
        ah_rigid(rh, l6, s, at_h);
#pragma unroll
        for (int k = 0; k < 6; ++k) lib[k] = at_h[k] - at_p[k];
        code = rk == 20 ? 3 : 4;
      }
      int k = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
          const double sym = 0.5 * ((double)row[a * 3 + b] + (double)row[b * 3 + a]);
          const double dd = d[a] * d[b];
          const double internal = stretch * dd + bend * ((a == b ? 1.0 : 0.0) - dd);
          const float value = (float)((sym + lib[k++]) + internal);
          out[a * 3 + b] = value;
          out[b * 3 + a] = value;
        }
      source[i] = code;
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) out[k] = NAN;
  source[i] = 0;
}

__global__ __launch_bounds__(WAVE) void cn_aniso_h_crystal_kernel(const int64_t* __restrict__ atom_ptr, int64_t N,
                                                                  const float* __restrict__ u_h,
                                                                  const int32_t* __restrict__ source,
                                                                  double* __restrict__ stats) {
  const int g = blockIdx.x, lane = threadIdx.x;
  int64_t a0, a1;
  cr_rows(atom_ptr, g, N, a0, a1);
  double nh = 0.0, tls = 0.0, sum = 0.0, bad = 0.0;
  for (int64_t a = a0 + lane; a < a1; a += WAVE) {
    const int32_t code = source[a];
    if (code < 2) continue;                                        // no hydrogen, or one without a tensor
    nh += 1.0;
    if (code >= 3) tls += 1.0;
    double t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = (double)u_h[(size_t)a * 9 + k];
    sum += ((t[0] + t[4]) + t[8]) / 3.0;
    const double m2 = t[0] * t[4] - t[1] * t[3];
    const double m3 = (t[0] * (t[4] * t[8] - t[5] * t[7]) - t[1] * (t[3] * t[8] - t[5] * t[6]))
                      + t[2] * (t[3] * t[7] - t[4] * t[6]);
    if (!(t[0] > 0.0 && m2 > 0.0 && m3 > 0.0)) bad += 1.0;         // Sylvester's criterion; a NaN is not positive
  }
  nh = cr_wave_sum(nh);
  tls = cr_wave_sum(tls);
  sum = cr_wave_sum(sum);
  bad = cr_wave_sum(bad);
  if (lane == 0) {
    stats[(size_t)g * 4 + 0] = nh;
    stats[(size_t)g * 4 + 1] = tls;
    stats[(size_t)g * 4 + 2] = sum;
    stats[(size_t)g * 4 + 3] = bad;
  }
}

}  // namespace

extern "C" int cartnet_adp_aniso_h(const float* u, const int64_t* z, const int64_t* edge_index, const float* cart_dist,
                                   const float* cart_dir, const int64_t* atom_row, const int64_t* seg_ptr,
                                   const int64_t* atom_ptr, const int64_t* parent, const double* x, const float* params,
                                   const int32_t* rank, double stretch, double bend, int32_t B, int64_t N, int64_t M,
                                   int64_t E, float* u_h, int32_t* source, double* crystal_stats, void* stream) {
  CN_CHECK(B >= 0 && N >= 0 && M >= 0 && E >= 0, "cartnet_adp_aniso_h: bad sizes (B=%d, N=%lld, M=%lld, E=%lld)", B,
           (long long)N, (long long)M, (long long)E);
  CN_CHECK(stretch == stretch && bend == bend, "cartnet_adp_aniso_h: stretch and bend must be numbers");
  CN_CHECK(N < (1LL << 31) * BG_ATOMS, "cartnet_adp_aniso_h: too many atoms for one launch");
  if (B == 0 || N == 0) return 0;
  CN_CHECK(z && atom_row && seg_ptr && parent && u_h && source, "cartnet_adp_aniso_h: null pointer");
  CN_CHECK(M == 0 || u, "cartnet_adp_aniso_h: null pointer");
  CN_CHECK(E == 0 || (edge_index && cart_dist && cart_dir), "cartnet_adp_aniso_h: null pointer");
  CN_CHECK(!crystal_stats || atom_ptr, "cartnet_adp_aniso_h: null pointer");
  CN_CHECK((x && params && rank) || (!x && !params && !rank),
           "cartnet_adp_aniso_h: x, params and rank come together or not at all");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((N + BG_ATOMS - 1) / BG_ATOMS));
  // without edges every segment is empty, without rows no hydrogen has a parent: the same launch writes the neutral values
  hipLaunchKernelGGL(cn_aniso_h_kernel, grid, dim3(BG_THREADS), 0, st, u, z, edge_index, cart_dist, cart_dir, atom_row,
                     seg_ptr, parent, x, params, rank, stretch, bend, N, M, E, u_h, source);
  CN_LAUNCH_CHECK("cartnet_adp_aniso_h");
  if (crystal_stats) {
    hipLaunchKernelGGL(cn_aniso_h_crystal_kernel, dim3(B), dim3(WAVE), 0, st, atom_ptr, N, u_h, source, crystal_stats);
    CN_LAUNCH_CHECK("cartnet_adp_aniso_h");
  }
  return 0;
}

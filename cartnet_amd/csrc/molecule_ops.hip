// Molecules of a batch's crystals from the bond graph, and the rigid-body test of Rosenfield, Trueblood & Dunitz (Acta
// Cryst. A34 (1978) 828) on predicted ADPs: Hirshfeld's postulate for ALL pairs of atoms of a molecule,
// D_ij = r^T U_i r / r.r - r^T U_j r / r.r ~ 0 along every interatomic vector r of a body that moves rigidly.  The
// reference has no counterpart: its only statements about a prediction need the truth (main.py:47-49).  The bond rule is
// that of bond_graph.h (bg_bond) with the target's crystal as the admissible range of sources: an edge whose source lies
// outside it is no bond (a well-formed batch has no such edge; one workgroup never reads what another writes).
//
//   cn_molecules_kernel       one workgroup per crystal, everything between two workgroup barriers, in five steps.
//     labels   Jacobi sweeps of "take the smallest label among the sources of my incoming bonds", the lowest edge among
//              those that carry it: two generations of int32 labels (an atom's index inside its crystal) ping-pong between
//              mol[] and mol_size[], the winning edge of an atom's LAST adoption (its offset in the atom's segment) sits in
//              mol_status[].  The sweeps end when no label changed and never run more than (atoms + 1) times.
//     x        At an atom's last adoption its source already held its final label, hence its final x: the Jacobi sum
//              x[i] = x[j] + fp64(dist) * fp64(dir) along the winning edge is the same fp64 additions whether it is
//              carried through the sweeps or taken along the finished tree, root first.  So x is written once per atom,
//              in sweeps of "my parent was done in an earlier sweep" (a stamp per row in mol[]); a sweep reads no x that
//              the same sweep writes.  Again at most (atoms + 1) sweeps.
//     flags    every bond edge once: different labels at its ends -> both molecules open; equal labels whose positions
//              disagree with the edge by more than 0.5 A -> periodic.  A molecule's two flags live at its root's row (in
//              mol_size[] and mol[]): plain stores of 1 by however many lanes.
//     rows     mol_status = periodic | 2 * open, then mol_size (atoms with my label) and mol (roots below mine) from the
//              finished labels: a scan of the crystal per atom, as the pair test below does anyway.
//     counts   crystal_counts[g] = (molecules, tested, periodic, open, largest size) over the roots, integer sums
//              folded through LDS in a fixed order.
//   cn_molecule_test_kernel   BG_LANES lanes per atom: they stride the atoms of its crystal, sixteen a pass, and keep
//                             those with its label.  Per pair, in fp64: r = x_i - x_j, D = r^T (S_i - S_j) r / r.r with S
//                             the symmetric part (the difference of the fp32 entries is taken first: exact in fp64); a
//                             pair with r.r == 0 is not counted.  The pairs of a pass are folded in ATOM order (bg_walk,
//                             bg_fold): sequential fp64 sums, a tie of |D| keeps the lower atom, a NaN is kept.  Rows of
//                             untested molecules (status != 0 or a single atom) get the neutral values without a pass.
//   cn_molecule_test_crystal_kernel   one wave per crystal: bg_pair_stats over the rows' pairs.
//
// No atomics, no workgroup waits for another, fixed order: two runs give the same bytes.  64-bit offsets throughout.
// No scratch; LDS only for the changed-flags of the sweeps and the five counts.
#include "bond_graph.h"

#include <limits.h>

namespace {

constexpr int MOL_THREADS = 256;
constexpr int MOL_WAVES = MOL_THREADS / WAVE;
constexpr double MOL_CLOSURE2 = 0.25;            // (0.5 A)^2: far above the rounding of x, far below a lattice translation

constexpr int MT_CHUNKS = 8;                     // workgroups per crystal: they stride its atoms, BG_ATOMS a pass

// the row of atom i, or -1
__device__ __forceinline__ int64_t mol_row(const BondGraph& g, int64_t i) { return bg_row(g.atom_row, i, g.M); }

// atom i's edge segment; empty for an atom that never bonds.  At most INT_MAX edges are looked at.
__device__ __forceinline__ void mol_segment(const BondGraph& g, int64_t i, int64_t zi, int64_t& e0, int64_t& e1) {
  bg_segment(g.seg_ptr, i, g.E, e0, e1);
  if (e1 - e0 > (int64_t)INT_MAX) e1 = e0 + INT_MAX;
  if (zi <= 1 || zi >= g.n_radii) e1 = e0;
}

__global__ __launch_bounds__(MOL_THREADS) void cn_molecules_kernel(
    const int64_t* __restrict__ z, const int64_t* __restrict__ src, const float* __restrict__ cart_dist,
    const float* __restrict__ cart_dir, const int64_t* __restrict__ atom_row, const int64_t* __restrict__ seg_ptr,
    const int64_t* __restrict__ ptr, const float* __restrict__ radii, int n_radii, float tol, int64_t N, int64_t M,
    int64_t E, int64_t* label, double* x, int32_t* mol, int32_t* mol_size, int32_t* mol_status,
    double* __restrict__ crystal_counts) {
  __shared__ int fold[MOL_WAVES][5];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
  const BondGraph g = {z, src, cart_dist, atom_row, seg_ptr, radii, n_radii, tol, N, M, E};
  int64_t a0, a1;                                                 // the crystal's atoms
  cr_rows(ptr, blockIdx.x, N, a0, a1);
  if (a1 - a0 > (int64_t)INT_MAX) a1 = a0 + INT_MAX;              // a label is an int32 index inside the crystal
  const int64_t n = a1 > a0 ? a1 - a0 : 0;

  // ---- labels: every atom with a row starts as its own
  int32_t* cur = mol;
  int32_t* nxt = mol_size;
  for (int64_t i = a0 + tid; i < a1; i += MOL_THREADS) {
    const int64_t m = mol_row(g, i);
    if (m >= 0) {
      cur[m] = (int32_t)(i - a0);
      nxt[m] = (int32_t)(i - a0);
      mol_status[m] = -1;                                         // no winning edge: a root
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int64_t sweep = 0; sweep <= n; ++sweep) {                  // the hard bound: atoms + 1
    int changed = 0;
    for (int64_t i = a0 + tid; i < a1; i += MOL_THREADS) {
      const int64_t m = mol_row(g, i);
      if (m < 0) continue;
      const int64_t zi = z[i];
      int64_t e0, e1;
      mol_segment(g, i, zi, e0, e1);
      const int32_t own = cur[m];
      int32_t best = own;
      int64_t at = -1;
      if (e1 > e0) {
        const float ri = radii[zi];
        for (int64_t e = e0; e < e1; ++e) {
          int64_t j, mj;
          if (!bg_bond(g, i, ri, e, a0, a1, j, mj)) continue;
          const int32_t lj = cur[mj];
          if (lj < best) {                                        // strictly: among equal labels the lowest edge stays
            best = lj;
            at = e;
          }
        }
      }
      nxt[m] = best;
      if (at >= 0) {
        mol_status[m] = (int32_t)(at - e0);
        changed = 1;
      }
    }
    __syncthreads();                                              // this sweep's stores, before the next sweep's loads
    const int any = __syncthreads_or(changed);
    int32_t* t = cur;
    cur = nxt;
    nxt = t;
    if (!any) break;
  }
  // cur holds the final labels (after a sweep without a change both generations are equal)
  for (int64_t i = a0 + tid; i < a1; i += MOL_THREADS) {
    const int64_t m = mol_row(g, i);
    label[i] = m >= 0 ? a0 + (int64_t)cur[m] : -1;
  }
  __syncthreads();

  // ---- x along the tree of winning edges, root first.  mol[] now holds the sweep in which a row was done.
  int32_t* done = mol;
  for (int64_t i = a0 + tid; i < a1; i += MOL_THREADS) {
    const int64_t m = mol_row(g, i);
    x[i * 3 + 0] = 0.0;
    x[i * 3 + 1] = 0.0;
    x[i * 3 + 2] = 0.0;
    if (m >= 0) done[m] = mol_status[m] < 0 ? 0 : INT_MAX;
  }
  __syncthreads();
#pragma unroll 1
  for (int64_t sweep = 1; sweep <= n + 1; ++sweep) {              // a tree of n atoms is n - 1 deep: the same hard bound
    const int32_t now = (int32_t)(sweep < INT_MAX ? sweep : INT_MAX - 1);
    int progress = 0;
    for (int64_t i = a0 + tid; i < a1; i += MOL_THREADS) {
      const int64_t m = mol_row(g, i);
      if (m < 0 || done[m] != INT_MAX) continue;
      int64_t e0, e1;
      mol_segment(g, i, z[i], e0, e1);
      const int64_t e = e0 + (int64_t)mol_status[m];
      if (e < e0 || e >= e1) continue;                            // cannot happen: the edge was chosen from this segment
      const int64_t j = src[e];
      if (j < a0 || j >= a1) continue;
      const int64_t mj = mol_row(g, j);
      if (mj < 0 || done[mj] >= now) continue;                    // the parent is not done, or only in this sweep
      const double d = (double)cart_dist[e];
#pragma unroll
      for (int q = 0; q < 3; ++q) x[i * 3 + q] = x[j * 3 + q] + d * (double)cart_dir[e * 3 + q];
      done[m] = now;
      progress = 1;
    }
    __syncthreads();
    if (!__syncthreads_or(progress)) break;
  }

  // ---- flags, at the root's row: periodic in mol_size[], open in mol[]
  for (int64_t i = a0 + tid; i < a1; i += MOL_THREADS) {
    const int64_t m = mol_row(g, i);
    if (m >= 0) {
      mol_size[m] = 0;
      mol[m] = 0;
    }
  }
  __syncthreads();
  for (int64_t i = a0 + tid; i < a1; i += MOL_THREADS) {
    const int64_t m = mol_row(g, i);
    if (m < 0) continue;
    const int64_t zi = z[i];
    int64_t e0, e1;
    mol_segment(g, i, zi, e0, e1);
    if (e1 <= e0) continue;
    const float ri = radii[zi];
    const int64_t li = label[i];
    const int64_t ri_row = mol_row(g, li);
    for (int64_t e = e0; e < e1; ++e) {
      int64_t j, mj;
      if (!bg_bond(g, i, ri, e, a0, a1, j, mj)) continue;
      const int64_t lj = label[j];
      if (lj != li) {
        const int64_t rj_row = (lj >= a0 && lj < a1) ? mol_row(g, lj) : -1;
        if (ri_row >= 0) mol[ri_row] = 1;
        if (rj_row >= 0) mol[rj_row] = 1;
      } else {
        const double d = (double)cart_dist[e];
        double gap2 = 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const double t = x[i * 3 + q] - (x[j * 3 + q] + d * (double)cart_dir[e * 3 + q]);
          gap2 += t * t;
        }
        if (gap2 > MOL_CLOSURE2 && ri_row >= 0) mol_size[ri_row] = 1;
      }
    }
  }
  __syncthreads();

  // ---- rows: the status first (it reads both flag arrays), then size and number (they read the labels only)
  for (int64_t i = a0 + tid; i < a1; i += MOL_THREADS) {
    const int64_t m = mol_row(g, i);
    if (m < 0) continue;
    const int64_t rr = mol_row(g, label[i]);
    mol_status[m] = rr >= 0 ? (mol_size[rr] ? 1 : 0) | (mol[rr] ? 2 : 0) : 0;
  }
  __syncthreads();
  for (int64_t i = a0 + tid; i < a1; i += MOL_THREADS) {
    const int64_t m = mol_row(g, i);
    if (m < 0) continue;
    const int64_t li = label[i];
    int32_t size = 0, below = 0;
    for (int64_t j = a0; j < a1; ++j) {
      const int64_t lj = label[j];
      size += lj == li ? 1 : 0;
      below += (lj == j && j < li) ? 1 : 0;
    }
    mol_size[m] = size;
    mol[m] = below;
  }
  __syncthreads();

  // ---- counts over the roots
  int c[5] = {0, 0, 0, 0, 0};
  for (int64_t i = a0 + tid; i < a1; i += MOL_THREADS) {
    const int64_t m = mol_row(g, i);
    if (m < 0 || label[i] != i) continue;
    const int32_t st = mol_status[m], sz = mol_size[m];
    c[0] += 1;
    c[1] += (st == 0 && sz >= 2) ? 1 : 0;
    c[2] += (st & 1) ? 1 : 0;
    c[3] += (st & 2) ? 1 : 0;
    c[4] = sz > c[4] ? sz : c[4];
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
      const int other = __shfl_xor(c[q], o);
      c[q] = q < 4 ? c[q] + other : (other > c[q] ? other : c[q]);
    }
    if (lane == 0) fold[wid][q] = c[q];
  }
  __syncthreads();
  if (tid < 5) {
    int v = fold[0][tid];
    for (int w = 1; w < MOL_WAVES; ++w) v = tid < 4 ? v + fold[w][tid] : (fold[w][tid] > v ? fold[w][tid] : v);
    crystal_counts[(size_t)blockIdx.x * 5 + tid] = (double)v;
  }
}

// r^T (S_i - S_j) r / r.r; r.r comes back in rr (0: the pair is not counted, the quotient not taken)
__device__ __forceinline__ double mt_delta(const double ui[9], const float* __restrict__ uj, const double xi[3],
                                           const double* xj, double& rr) {
  double w[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) w[q] = ui[q] - (double)uj[q];
  const double a = xi[0] - xj[0], b = xi[1] - xj[1], c = xi[2] - xj[2];
  rr = a * a + b * b + c * c;
  const double form = bg_form(w, a, b, c);
  return rr == 0.0 ? 0.0 : form / rr;
}

__global__ __launch_bounds__(BG_THREADS) void cn_molecule_test_kernel(
    const float* __restrict__ u, const int64_t* __restrict__ label, const double* __restrict__ x,
    const int64_t* __restrict__ atom_row, const int64_t* __restrict__ ptr, const int32_t* __restrict__ mol_status,
    const int32_t* __restrict__ mol_size, double threshold, int64_t N, int64_t M, int32_t* __restrict__ pairs,
    float* __restrict__ delta_sum, float* __restrict__ delta_max, int64_t* __restrict__ worst,
    int32_t* __restrict__ over) {
  const int lane = threadIdx.x & (WAVE - 1), sub = lane & (BG_LANES - 1), base = lane - sub;
  int64_t a0, a1;
  cr_rows(ptr, blockIdx.x, N, a0, a1);
#pragma unroll 1
  for (int64_t first = a0 + (int64_t)blockIdx.y * BG_ATOMS; first < a1; first += (int64_t)MT_CHUNKS * BG_ATOMS) {
    const int64_t i = first + (threadIdx.x / BG_LANES);
    int64_t m = -1, li = -1;
    if (i < a1) m = bg_row(atom_row, i, M);                        // -1: nothing to write
    bool tested = false;
    if (m >= 0) {
      li = label[i];
      tested = mol_status[m] == 0 && mol_size[m] >= 2 && li >= 0;
    }
    double ui[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, xi[3] = {0.0, 0.0, 0.0};
    if (tested) {
#pragma unroll
      for (int q = 0; q < 9; ++q) ui[q] = (double)u[m * 9 + q];
#pragma unroll
      for (int q = 0; q < 3; ++q) xi[q] = x[i * 3 + q];
    }
    BgFold f;
    const int64_t c1 = tested ? a1 : a0;                          // an untested row makes no pass
#pragma unroll 1
    for (int64_t c = a0; c < c1; c += BG_LANES) {
      const int64_t j = c + sub;
      bool pair = false;
      double a = 0.0;
      if (j < a1 && j != i && label[j] == li) {
        const int64_t mj = bg_row(atom_row, j, M);
        if (mj >= 0) {
          double rr;
          a = fabs(mt_delta(ui, u + mj * 9, xi, x + j * 3, rr));
          pair = rr != 0.0;
        }
      }
      // the pairs of this pass, lowest atom first
      bg_walk(pair, base, [&](int l) { bg_fold(f, __shfl(a, l), __shfl((long long)j, l), threshold); });
    }
    if (m >= 0 && sub == 0) {
      pairs[m] = f.n;
      delta_sum[m] = (float)f.sum;
      delta_max[m] = (float)f.hi;
      worst[m] = f.who;
      over[m] = f.over;
    }
  }
}

__global__ __launch_bounds__(WAVE) void cn_molecule_test_crystal_kernel(const int64_t* __restrict__ row_ptr, int64_t M,
                                                                        const int32_t* __restrict__ pairs,
                                                                        const float* __restrict__ delta_sum,
                                                                        const float* __restrict__ delta_max,
                                                                        const int32_t* __restrict__ over,
                                                                        double* __restrict__ stats) {
  bg_pair_stats(row_ptr, M, pairs, delta_sum, delta_max, over, stats);
}

}  // namespace

extern "C" int cartnet_molecules(const int64_t* z, const int64_t* edge_index, const float* cart_dist, const float* cart_dir,
                                 const int64_t* atom_row, const int64_t* seg_ptr, const int64_t* ptr,
                                 const int64_t* row_ptr, const float* radii, int32_t n_radii, float tol, int32_t B,
                                 int64_t N, int64_t M, int64_t E, int64_t* label, double* x, int32_t* mol,
                                 int32_t* mol_size, int32_t* mol_status, double* crystal_counts, void* stream) {
  CN_CHECK(B >= 0 && N >= 0 && M >= 0 && E >= 0 && n_radii >= 0,
           "cartnet_molecules: bad sizes (B=%d, N=%lld, M=%lld, E=%lld, n_radii=%d)", B, (long long)N, (long long)M,
           (long long)E, n_radii);
  CN_CHECK(tol == tol, "cartnet_molecules: tol must be a number");
  if (M == 0 || B == 0 || N == 0) return 0;
  CN_CHECK(z && atom_row && seg_ptr && ptr && row_ptr && label && x && mol && mol_size && mol_status && crystal_counts,
           "cartnet_molecules: null pointer");
  CN_CHECK(E == 0 || (edge_index && cart_dist && cart_dir && radii), "cartnet_molecules: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // without edges every segment is empty: every atom with a row is a molecule of its own, from the same launch
  hipLaunchKernelGGL(cn_molecules_kernel, dim3((unsigned)B), dim3(MOL_THREADS), 0, st, z, edge_index, cart_dist, cart_dir,
                     atom_row, seg_ptr, ptr, radii, (int)n_radii, tol, N, M, E, label, x, mol, mol_size, mol_status,
                     crystal_counts);
  CN_LAUNCH_CHECK("cartnet_molecules");
  return 0;
}

extern "C" int cartnet_adp_molecule_test(const float* u, const int64_t* label, const double* x, const int64_t* atom_row,
                                         const int64_t* ptr, const int64_t* row_ptr, const int32_t* mol_status,
                                         const int32_t* mol_size, double threshold, int32_t B, int64_t N, int64_t M,
                                         int32_t* pairs, float* delta_sum, float* delta_max, int64_t* worst, int32_t* over,
                                         double* crystal_stats, void* stream) {
  CN_CHECK(B >= 0 && N >= 0 && M >= 0, "cartnet_adp_molecule_test: bad sizes (B=%d, N=%lld, M=%lld)", B, (long long)N,
           (long long)M);
  CN_CHECK(threshold == threshold, "cartnet_adp_molecule_test: threshold must be a number");
  if (M == 0 || B == 0 || N == 0) return 0;
  CN_CHECK(u && label && x && atom_row && ptr && row_ptr && mol_status && mol_size && pairs && delta_sum && delta_max &&
               worst && over,
           "cartnet_adp_molecule_test: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cn_molecule_test_kernel, dim3((unsigned)B, MT_CHUNKS), dim3(BG_THREADS), 0, st, u, label, x, atom_row,
                     ptr, mol_status, mol_size, threshold, N, M, pairs, delta_sum, delta_max, worst, over);
  CN_LAUNCH_CHECK("cartnet_adp_molecule_test");
  if (crystal_stats) {
    hipLaunchKernelGGL(cn_molecule_test_crystal_kernel, dim3(B), dim3(WAVE), 0, st, row_ptr, M, pairs, delta_sum,
                       delta_max, over, crystal_stats);
    CN_LAUNCH_CHECK("cartnet_adp_molecule_test");
  }
  return 0;
}

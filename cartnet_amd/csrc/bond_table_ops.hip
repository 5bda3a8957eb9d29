// The bond table of predicted ADPs: one entry per bond of a crystal instead of the per-atom aggregates of bond_ops.hip --
// Hirshfeld's D with its sign, the Busing & Levy (1964) bounds on the thermally averaged bond length, and the bond length
// corrected for the libration of a fitted rigid body (Cruickshank 1956; Schomaker & Trueblood 1968), which is what THMA11
// and PLATON print after a TLS analysis.  The reference has no counterpart.  cartnet_amd/bonds.py states the rule and
// restates both kernels in numpy (bond_table_host).
//
// A directed edge e = (j -> i) is a bond by the rule of bond_graph.h (bg_bond), exactly as in bond_ops.hip; the table
// lists the bonds with j < i, in target order and within a target in edge order: the graph's own order.  A table has a
// length nobody knows before the graph is read, so there are two entry points with a static-shape scan between them:
//
//   cn_bond_table_count_kernel    BG_LANES lanes per atom stride its edge segment; per pass the group counts the lanes
//                                 whose edge is a bond with j < i (listed) and with j > i (unlisted: a capped graph can
//                                 hold a bond in one direction only).  It does not read U.
//   cn_bond_table_fill_kernel     the same walk with the atom's exclusive offset: a lane's slot is the offset, plus the
//                                 listed bonds of the earlier passes, plus the lower lanes of its group that raised the
//                                 flag in this pass (the ballot bg_walk takes).  Every listed lane then computes and
//                                 stores its own entry; nothing is folded, so no lane waits for another.  Per entry, in
//                                 fp64 from the fp32 inputs and rounded once on store, with a = j, b = i, d and l as
//                                 stored:  delta = d^T (Sym U_b - Sym U_a) d (the difference first, bg_form: the
//                                 expression of bond_ops.hip under the same contraction);  w_x^2 = tr U_x - d^T Sym U_x d;
//                                 lower / upper = l + (sqrt w_b^2 -/+ sqrt w_a^2)^2 / (2 l), NaN where a w^2 is negative
//                                 or NaN (the square root's own answer);  libration = |r + (tr(L) r - L r) / 2|, r = l d,
//                                 L from row b's TLS parameters as stored, where that row's rank is > 0.
//   cn_bond_table_crystal_kernel  one wave per crystal over its entries as stored (crystal_reduce.h) and over its atoms'
//                                 unlisted counts.
//
// No atomics, no workgroup waits for another, fixed order: two runs give the same bytes.  64-bit offsets throughout; a slot
// is compared with the table's length before anything is stored.  No kernel uses scratch or LDS.
#include "bond_graph.h"

namespace {

// what a group's lanes share about their atom: its row (or -1), its radius and its edge segment (empty when never bonded)
struct BtAtom {
  int64_t i, m, e0, e1;
  float ri;
};

__device__ __forceinline__ BtAtom bt_atom(const BondGraph& g) {
  BtAtom a = {(int64_t)blockIdx.x * BG_ATOMS + (threadIdx.x / BG_LANES), -1, 0, 0, 0.f};
  if (a.i < g.N) a.m = bg_row(g.atom_row, a.i, g.M);
  if (a.m >= 0) {
    const int64_t zi = g.z[a.i];
    bg_segment(g.seg_ptr, a.i, g.E, a.e0, a.e1);
    if (zi <= 1 || zi >= g.n_radii) a.e1 = a.e0;                  // hydrogen, 0 or beyond the table: never bonded
    if (a.e1 > a.e0) a.ri = g.radii[zi];
  }
  return a;
}

// the flags of the group at `base`, lane `sub` of the group in bit `sub`
__device__ __forceinline__ unsigned int bt_flags(bool flag, int base) {
  return (unsigned int)((__ballot(flag) >> base) & ((1ull << BG_LANES) - 1));
}

__global__ __launch_bounds__(BG_THREADS) void cn_bond_table_count_kernel(
    const int64_t* __restrict__ z, const int64_t* __restrict__ src, const float* __restrict__ cart_dist,
    const int64_t* __restrict__ atom_row, const int64_t* __restrict__ seg_ptr, const float* __restrict__ radii,
    int n_radii, float tol, int64_t N, int64_t M, int64_t E, int32_t* __restrict__ listed,
    int32_t* __restrict__ unlisted) {
  const BondGraph g = {z, src, cart_dist, atom_row, seg_ptr, radii, n_radii, tol, N, M, E};
  const int lane = threadIdx.x & (WAVE - 1), sub = lane & (BG_LANES - 1), base = lane - sub;
  const BtAtom a = bt_atom(g);
  int32_t n = 0, other = 0;
#pragma unroll 1
  for (int64_t c = a.e0; c < a.e1; c += BG_LANES) {
    const int64_t e = c + sub;
    int64_t j = -1, mj = -1;
    const bool bond = e < a.e1 && bg_bond(g, a.i, a.ri, e, 0, N, j, mj);
    n += __popc(bt_flags(bond && j < a.i, base));
    other += __popc(bt_flags(bond && j > a.i, base));
  }
  if (a.i < N && sub == 0) {
    listed[a.i] = n;
    unlisted[a.i] = other;
  }
}

__global__ __launch_bounds__(BG_THREADS) void cn_bond_table_fill_kernel(
    const float* __restrict__ u, const int64_t* __restrict__ z, const int64_t* __restrict__ src,
    const float* __restrict__ cart_dist, const float* __restrict__ cart_dir, const int64_t* __restrict__ atom_row,
    const int64_t* __restrict__ seg_ptr, const float* __restrict__ radii, int n_radii, float tol,
    const int64_t* __restrict__ offset, const float* __restrict__ params, const int32_t* __restrict__ rank, int64_t N,
    int64_t M, int64_t E, int64_t nb, int64_t* __restrict__ out_a, int64_t* __restrict__ out_b,
    float* __restrict__ out_dir, float* __restrict__ length, float* __restrict__ delta, float* __restrict__ lower,
    float* __restrict__ upper, float* __restrict__ libration, int32_t* __restrict__ tls_rank) {
  const BondGraph g = {z, src, cart_dist, atom_row, seg_ptr, radii, n_radii, tol, N, M, E};
  const int lane = threadIdx.x & (WAVE - 1), sub = lane & (BG_LANES - 1), base = lane - sub;
  const BtAtom a = bt_atom(g);
  int64_t slot = a.e1 > a.e0 ? offset[a.i] : 0;
#pragma unroll 1
  for (int64_t c = a.e0; c < a.e1; c += BG_LANES) {
    const int64_t e = c + sub;
    int64_t j = -1, mj = -1;
    const bool mine = e < a.e1 && bg_bond(g, a.i, a.ri, e, 0, N, j, mj) && j < a.i;
    const unsigned int found = bt_flags(mine, base);
    const int64_t s = slot + __popc(found & ((1u << sub) - 1u));
    slot += __popc(found);
    if (!mine || s < 0 || s >= nb) continue;                       // a slot outside the table is never written
    double ub[9], ua[9], w[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      ub[q] = (double)u[a.m * 9 + q];
      ua[q] = (double)u[mj * 9 + q];
      w[q] = ub[q] - ua[q];
    }
    const float* __restrict__ dir = cart_dir + e * 3;
    const double x = (double)dir[0], y = (double)dir[1], zz = (double)dir[2], l = (double)cart_dist[e];
    const double wb = sqrt((ub[0] + ub[4] + ub[8]) - bg_form(ub, x, y, zz));
    const double wa = sqrt((ua[0] + ua[4] + ua[8]) - bg_form(ua, x, y, zz));
    const double lo = wb - wa, hi = wb + wa;
    out_a[s] = j;
    out_b[s] = a.i;
    out_dir[s * 3 + 0] = dir[0];
    out_dir[s * 3 + 1] = dir[1];
    out_dir[s * 3 + 2] = dir[2];
    length[s] = cart_dist[e];
    delta[s] = (float)bg_form(w, x, y, zz);
    lower[s] = (float)(l + lo * lo / (2.0 * l));
    upper[s] = (float)(l + hi * hi / (2.0 * l));
    const int32_t rk = rank ? rank[a.m] : 0;
    float lib = NAN;
    if (params && rk > 0) {
      const float* __restrict__ p = params + a.m * 24 + 6;          // L: 11 22 33 23 13 12
      const double l11 = (double)p[0], l22 = (double)p[1], l33 = (double)p[2], l23 = (double)p[3], l13 = (double)p[4],
                   l12 = (double)p[5];
      const double rx = l * x, ry = l * y, rz = l * zz, t = l11 + l22 + l33;
      const double vx = rx + 0.5 * (t * rx - (l11 * rx + l12 * ry + l13 * rz));
      const double vy = ry + 0.5 * (t * ry - (l12 * rx + l22 * ry + l23 * rz));
      const double vz = rz + 0.5 * (t * rz - (l13 * rx + l23 * ry + l33 * rz));
      lib = (float)sqrt(vx * vx + vy * vy + vz * vz);
    }
    libration[s] = lib;
    tls_rank[s] = rk;
  }
}

// stats[g] = (listed, unlisted, sum of length, sum of |delta|, largest |delta| -- it keeps a NaN --, entries with a finite
// libration, sum and largest of libration - length over those (0 without one), entries with a NaN bound)
__global__ __launch_bounds__(WAVE) void cn_bond_table_crystal_kernel(
    const int64_t* __restrict__ atom_ptr, const int64_t* __restrict__ offset, const int32_t* __restrict__ unlisted,
    int64_t N, int64_t nb, const float* __restrict__ length, const float* __restrict__ delta,
    const float* __restrict__ lower, const float* __restrict__ upper, const float* __restrict__ libration,
    double* __restrict__ stats) {
  const int g = blockIdx.x, lane = threadIdx.x;
  int64_t a0, a1, b0, b1;
  cr_rows(atom_ptr, g, N, a0, a1);
  a0 = a0 > N ? N : a0;                                            // offset has N + 1 entries
  a1 = a1 < a0 ? a0 : a1;
  b0 = offset[a0];
  b1 = offset[a1];
  b0 = b0 < 0 ? 0 : b0;
  b1 = b1 > nb ? nb : b1;
  double other = 0.0, len = 0.0, sum = 0.0, hi = 0.0, nl = 0.0, grow = 0.0, top = -INFINITY, bad = 0.0;
  for (int64_t i = a0 + lane; i < a1; i += WAVE) other += (double)unlisted[i];
  for (int64_t s = b0 + lane; s < b1; s += WAVE) {
    const double l = (double)length[s], d = fabs((double)delta[s]), lib = (double)libration[s];
    len += l;
    sum += d;
    hi = cr_max_nan(hi, d);
    if (lib - lib == 0.0) {                                        // finite
      nl += 1.0;
      grow += lib - l;
      top = cr_max_nan(top, lib - l);
    }
    bad += (lower[s] != lower[s] || upper[s] != upper[s]) ? 1.0 : 0.0;
  }
  other = cr_wave_sum(other);
  len = cr_wave_sum(len);
  sum = cr_wave_sum(sum);
  hi = cr_wave_max_nan(hi);
  nl = cr_wave_sum(nl);
  grow = cr_wave_sum(grow);
  top = cr_wave_max_nan(top);
  bad = cr_wave_sum(bad);
  if (lane == 0) {
    double* __restrict__ o = stats + (size_t)g * 9;
    o[0] = (double)(b1 > b0 ? b1 - b0 : 0);
    o[1] = other;
    o[2] = len;
    o[3] = sum;
    o[4] = hi;
    o[5] = nl;
    o[6] = grow;
    o[7] = nl > 0.0 ? top : 0.0;
    o[8] = bad;
  }
}

}  // namespace

extern "C" int cartnet_bond_table_count(const int64_t* z, const int64_t* edge_index, const float* cart_dist,
                                        const int64_t* atom_row, const int64_t* seg_ptr, const float* radii,
                                        int32_t n_radii, float tol, int64_t N, int64_t M, int64_t E, int32_t* listed,
                                        int32_t* unlisted, void* stream) {
  CN_CHECK(N >= 0 && M >= 0 && E >= 0 && n_radii >= 0, "cartnet_bond_table_count: bad sizes (N=%lld, M=%lld, E=%lld, "
           "n_radii=%d)", (long long)N, (long long)M, (long long)E, n_radii);
  CN_CHECK(tol == tol, "cartnet_bond_table_count: tol must be a number");
  CN_CHECK(N < (1LL << 31) * BG_ATOMS, "cartnet_bond_table_count: too many atoms for one launch");
  if (N == 0) return 0;
  CN_CHECK(z && atom_row && seg_ptr && listed && unlisted, "cartnet_bond_table_count: null pointer");
  CN_CHECK(E == 0 || (edge_index && cart_dist && radii), "cartnet_bond_table_count: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // without edges (or without rows) every segment is empty: the atoms get their zeros from the same launch
  hipLaunchKernelGGL(cn_bond_table_count_kernel, dim3((unsigned)((N + BG_ATOMS - 1) / BG_ATOMS)), dim3(BG_THREADS), 0, st,
                     z, edge_index, cart_dist, atom_row, seg_ptr, radii, (int)n_radii, tol, N, M, E, listed, unlisted);
  CN_LAUNCH_CHECK("cartnet_bond_table_count");
  return 0;
}

extern "C" int cartnet_adp_bond_table(const float* u, const int64_t* z, const int64_t* edge_index, const float* cart_dist,
                                      const float* cart_dir, const int64_t* atom_row, const int64_t* seg_ptr,
                                      const int64_t* atom_ptr, const float* radii, int32_t n_radii, float tol,
                                      const int64_t* offset, const int32_t* unlisted, const float* params,
                                      const int32_t* rank, int32_t B, int64_t N, int64_t M, int64_t E, int64_t nb,
                                      int64_t* a, int64_t* b, float* dir, float* length, float* delta, float* lower,
                                      float* upper, float* libration, int32_t* tls_rank, double* crystal_stats,
                                      void* stream) {
  CN_CHECK(B >= 0 && N >= 0 && M >= 0 && E >= 0 && nb >= 0 && n_radii >= 0,
           "cartnet_adp_bond_table: bad sizes (B=%d, N=%lld, M=%lld, E=%lld, nb=%lld, n_radii=%d)", B, (long long)N,
           (long long)M, (long long)E, (long long)nb, n_radii);
  CN_CHECK(tol == tol, "cartnet_adp_bond_table: tol must be a number");
  CN_CHECK(N < (1LL << 31) * BG_ATOMS, "cartnet_adp_bond_table: too many atoms for one launch");
  CN_CHECK((params == nullptr) == (rank == nullptr), "cartnet_adp_bond_table: params and rank come together or not at all");
  if (B == 0 || N == 0) return 0;
  CN_CHECK(z && atom_row && seg_ptr && atom_ptr && offset && unlisted, "cartnet_adp_bond_table: null pointer");
  CN_CHECK(nb == 0 || (u && edge_index && cart_dist && cart_dir && radii && a && b && dir && length && delta && lower &&
                       upper && libration && tls_rank && M > 0 && E > 0),
           "cartnet_adp_bond_table: null pointer (a table of %lld entries needs u, the edges and every output)",
           (long long)nb);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (nb > 0) {
    hipLaunchKernelGGL(cn_bond_table_fill_kernel, dim3((unsigned)((N + BG_ATOMS - 1) / BG_ATOMS)), dim3(BG_THREADS), 0, st,
                       u, z, edge_index, cart_dist, cart_dir, atom_row, seg_ptr, radii, (int)n_radii, tol, offset, params,
                       rank, N, M, E, nb, a, b, dir, length, delta, lower, upper, libration, tls_rank);
    CN_LAUNCH_CHECK("cartnet_adp_bond_table");
  }
  if (crystal_stats) {
    hipLaunchKernelGGL(cn_bond_table_crystal_kernel, dim3(B), dim3(WAVE), 0, st, atom_ptr, offset, unlisted, N, nb, length,
                       delta, lower, upper, libration, crystal_stats);
    CN_LAUNCH_CHECK("cartnet_adp_bond_table");
  }
  return 0;
}

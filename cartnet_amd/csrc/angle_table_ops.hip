// The angle and torsion tables of a batch: the valence angles a-b-c and the torsions a-b-c-d of the bond graph, from the
// edges of the radius graph alone (cart_dir, cart_dist: never pos, so cell faces and images need no special case), each
// with the value that the libration L of a fitted rigid body gives (v' = v + (tr(L) v - L v) / 2 on every bond vector:
// what THMA11 and PLATON print beside the corrected distances).  The reference has no counterpart.  cartnet_amd/bonds.py
// states the rule and restates every kernel in numpy (angle_table_host).
//
// This file is compiled with -ffp-contract=off (build.py) and does not call bg_form: with the stored fp32 values as
// inputs every product, sum and square root below is the fp64 (for the reverse edge: fp32) value numpy computes, in the
// same order; only atan2's last bits can differ.
//
// A directed edge e = (j -> i) is a bond by bg_bond, as in bond_table_ops.hip.  Atom i's adjacency is the bond edges of its
// segment in edge order (ascending edge index), sources below and above i alike; its degree is listed + unlisted of
// cartnet_bond_table_count, and nbr_ptr their exclusive scan.  Variable-length output at two levels, so: lists, counts,
// a scan on the host side (static shapes), fills.
//
//   cn_bond_adjacency_kernel   BG_LANES lanes per atom walk its edge segment as cn_bond_table_fill_kernel does; a lane's
//                              slot comes from its group's ballot.  adj[nbr_ptr[i] + k]: the k-th bond edge of i;
//                              bond_edge[offset[i] + k']: the edge of i's k'-th listed bond (j < i), the bond table's row.
//   cn_angle_count_kernel      per atom d (d - 1) / 2; per listed bond e0 = (b -> c), by the group of c: the reverse edge
//                              -- among the bond edges e' of b's adjacency with source c the one with the smallest
//                              max_k |fp32(l' d'_k + l0 d0_k)|, the lanes striding b's adjacency and bg_argmin folding
//                              (a tie: the lowest edge), accepted below 0.5 A --, and n_a n_d with n_d = d_c - 1 and n_a =
//                              d_b less the reverse edge if there is one.
//   cn_angle_fill_kernel       the group of centre b: lanes stride k1, every lane loops k2 > k1; the slot inside the atom
//                              is k1 (2 d - k1 - 1) / 2 + (k2 - k1 - 1).
//   cn_torsion_fill_kernel     the group of atom c takes c's listed bonds in turn; lanes stride the n_a n_d products, slot
//                              ia n_d + id.  The ia-th edge of b's adjacency without the reverse edge is adj[ia], or
//                              adj[ia + 1] from the reverse edge on (the adjacency ascends); the same for id and e0.
//   cn_angle_table_crystal_kernel  one wave per crystal over its entries as stored (crystal_reduce.h).
//
// No atomics, no LDS, no scratch, no workgroup waits for another, fixed order: two runs give the same bytes.  64-bit
// offsets throughout (bg_segment cuts an atom's piece out of any of the exclusive scans, clamped to its list); a slot is
// compared with its table's length, an edge read from a list with E and an atom with N before anything is stored or
// dereferenced.  A wave holds four whole groups, and every loop that holds a ballot or a shuffle has bounds that the lanes
// of a group share.
#include "bond_graph.h"

namespace {

constexpr double AT_DEGREES = 57.29577951308232;                   // 180 / pi
constexpr float AT_CLOSURE = 0.5f;                                 // bonds.MOLECULE_CLOSURE

struct AtVec {
  double x, y, z;
};

__device__ __forceinline__ AtVec at_cross(const AtVec& p, const AtVec& q) {
  return {p.y * q.z - p.z * q.y, p.z * q.x - p.x * q.z, p.x * q.y - p.y * q.x};
}

__device__ __forceinline__ double at_dot(const AtVec& p, const AtVec& q) { return (p.x * q.x + p.y * q.y) + p.z * q.z; }

// the stored unit direction of edge e, and the bond vector l d
__device__ __forceinline__ AtVec at_dir(const float* __restrict__ cart_dir, int64_t e) {
  return {(double)cart_dir[e * 3 + 0], (double)cart_dir[e * 3 + 1], (double)cart_dir[e * 3 + 2]};
}

__device__ __forceinline__ AtVec at_scaled(const AtVec& d, double l) { return {l * d.x, l * d.y, l * d.z}; }

// L of a row's TLS parameters as stored (11 22 33 23 13 12), or nothing
struct AtLib {
  bool on;
  int32_t rank;
  double l11, l22, l33, l23, l13, l12;
};

__device__ __forceinline__ AtLib at_lib(const float* __restrict__ params, const int32_t* __restrict__ rank, int64_t m) {
  AtLib t = {false, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (m < 0 || !rank) return t;
  t.rank = rank[m];
  if (!params || t.rank <= 0) return t;
  const float* __restrict__ p = params + m * 24 + 6;
  t.on = true;
  t.l11 = (double)p[0], t.l22 = (double)p[1], t.l33 = (double)p[2];
  t.l23 = (double)p[3], t.l13 = (double)p[4], t.l12 = (double)p[5];
  return t;
}

// v + (tr(L) v - L v) / 2, in the operation order of cn_bond_table_fill_kernel
__device__ __forceinline__ AtVec at_librated(const AtLib& t, const AtVec& r) {
  const double tr = (t.l11 + t.l22) + t.l33;
  return {r.x + 0.5 * (tr * r.x - ((t.l11 * r.x + t.l12 * r.y) + t.l13 * r.z)),
          r.y + 0.5 * (tr * r.y - ((t.l12 * r.x + t.l22 * r.y) + t.l23 * r.z)),
          r.z + 0.5 * (tr * r.z - ((t.l13 * r.x + t.l23 * r.y) + t.l33 * r.z))};
}

// the angle of p and q in degrees: atan2(|p x q|, p . q)
__device__ __forceinline__ float at_angle(const AtVec& p, const AtVec& q) {
  const AtVec c = at_cross(p, q);
  return (float)(atan2(sqrt(at_dot(c, c)), at_dot(p, q)) * AT_DEGREES);
}

// the torsion of b1, b2, b3 in degrees with the IUPAC sign: atan2(|b2| b1 . n2, n1 . n2); an fp32 -180 is +180
__device__ __forceinline__ float at_torsion(const AtVec& b1, const AtVec& b2, const AtVec& b3, bool& defined) {
  const AtVec n1 = at_cross(b1, b2), n2 = at_cross(b2, b3);
  defined = !(at_dot(n1, n1) == 0.0 || at_dot(n2, n2) == 0.0);
  const float v = (float)(atan2(sqrt(at_dot(b2, b2)) * at_dot(b1, n2), at_dot(n1, n2)) * AT_DEGREES);
  return v == -180.f ? 180.f : v;
}

__global__ __launch_bounds__(BG_THREADS) void cn_bond_adjacency_kernel(
    const int64_t* __restrict__ z, const int64_t* __restrict__ src, const float* __restrict__ cart_dist,
    const int64_t* __restrict__ atom_row, const int64_t* __restrict__ seg_ptr, const float* __restrict__ radii,
    int n_radii, float tol, const int64_t* __restrict__ nbr_ptr, const int64_t* __restrict__ offset, int64_t N, int64_t M,
    int64_t E, int64_t nb, int64_t* __restrict__ adj, int64_t* __restrict__ bond_edge) {
  const BondGraph g = {z, src, cart_dist, atom_row, seg_ptr, radii, n_radii, tol, N, M, E};
  const int lane = threadIdx.x & (WAVE - 1), sub = lane & (BG_LANES - 1), base = lane - sub;
  const int64_t i = (int64_t)blockIdx.x * BG_ATOMS + (threadIdx.x / BG_LANES);
  int64_t e0 = 0, e1 = 0;
  float ri = 0.f;
  if (i < N && bg_row(atom_row, i, M) >= 0) {
    const int64_t zi = z[i];
    bg_segment(seg_ptr, i, E, e0, e1);
    if (zi <= 1 || zi >= n_radii) e1 = e0;                         // hydrogen, 0 or beyond the table: never bonded
    if (e1 > e0) ri = radii[zi];
  }
  int64_t all = e1 > e0 ? nbr_ptr[i] : 0, listed = e1 > e0 ? offset[i] : 0;
#pragma unroll 1
  for (int64_t c = e0; c < e1; c += BG_LANES) {
    const int64_t e = c + sub;
    int64_t j = -1, mj = -1;
    const bool bond = e < e1 && bg_bond(g, i, ri, e, 0, N, j, mj);
    const bool low = bond && j < i;
    const unsigned int fa = bg_flags(bond, base), fl = bg_flags(low, base), below = (1u << sub) - 1u;
    const int64_t sa = all + __popc(fa & below), sl = listed + __popc(fl & below);
    all += __popc(fa);
    listed += __popc(fl);
    if (bond && sa >= 0 && sa < E) adj[sa] = e;                    // a slot outside a list is never written
    if (low && sl >= 0 && sl < nb) bond_edge[sl] = e;
  }
}

__global__ __launch_bounds__(BG_THREADS) void cn_angle_count_kernel(
    const int64_t* __restrict__ src, const float* __restrict__ cart_dist, const float* __restrict__ cart_dir,
    const int64_t* __restrict__ nbr_ptr, const int64_t* __restrict__ offset, const int64_t* __restrict__ adj,
    const int64_t* __restrict__ bond_edge, int64_t N, int64_t E, int64_t nb, int64_t* __restrict__ angle_count,
    int64_t* __restrict__ reverse, int64_t* __restrict__ torsion_count) {
  const int lane = threadIdx.x & (WAVE - 1), sub = lane & (BG_LANES - 1);
  const int64_t i = (int64_t)blockIdx.x * BG_ATOMS + (threadIdx.x / BG_LANES);
  int64_t p0 = 0, p1 = 0, k0 = 0, k1 = 0;
  if (i < N) {
    bg_segment(nbr_ptr, i, E, p0, p1);
    bg_segment(offset, i, nb, k0, k1);
  }
  const int64_t d = p1 - p0;
  if (i < N && sub == 0) angle_count[i] = d * (d - 1) / 2;
#pragma unroll 1
  for (int64_t kb = k0; kb < k1; ++kb) {                           // the listed bonds e0 = (b -> i) of this atom
    const int64_t e0 = bond_edge[kb];
    int64_t b = (e0 >= 0 && e0 < E) ? src[e0] : -1, q0 = 0, q1 = 0;
    if (b < 0 || b >= N) b = -1;
    float l0 = 0.f, x0 = 0.f, y0 = 0.f, z0 = 0.f;
    if (b >= 0) {
      bg_segment(nbr_ptr, b, E, q0, q1);
      l0 = cart_dist[e0], x0 = cart_dir[e0 * 3 + 0], y0 = cart_dir[e0 * 3 + 1], z0 = cart_dir[e0 * 3 + 2];
    }
    float best = INFINITY;
    int64_t at = E;
#pragma unroll 1
    for (int64_t c = q0; c < q1; c += BG_LANES) {
      const int64_t e = c + sub < q1 ? adj[c + sub] : -1;
      if (e < 0 || e >= E || src[e] != i) continue;
      const float l = cart_dist[e];
      const float sx = fabsf(l * cart_dir[e * 3 + 0] + l0 * x0), sy = fabsf(l * cart_dir[e * 3 + 1] + l0 * y0),
                  sz = fabsf(l * cart_dir[e * 3 + 2] + l0 * z0);
      float m = sx;
      m = sy > m ? sy : m;
      m = sz > m ? sz : m;
      if (m < best) {                                              // ascending edges: a tie keeps the lowest
        best = m;
        at = e;
      }
    }
    bg_argmin(best, at, E);
    const int64_t rev = (at < E && best < AT_CLOSURE) ? at : -1;
    if (sub == 0) {
      reverse[kb] = rev;
      torsion_count[kb] = b >= 0 ? ((q1 - q0) - (rev >= 0 ? 1 : 0)) * (d - 1) : 0;
    }
  }
}

__global__ __launch_bounds__(BG_THREADS) void cn_angle_fill_kernel(
    const int64_t* __restrict__ src, const float* __restrict__ cart_dist, const float* __restrict__ cart_dir,
    const int64_t* __restrict__ atom_row, const int64_t* __restrict__ nbr_ptr, const int64_t* __restrict__ adj,
    const int64_t* __restrict__ angle_offset, const float* __restrict__ params, const int32_t* __restrict__ rank,
    int64_t N, int64_t M, int64_t E, int64_t na, int64_t* __restrict__ out_a, int64_t* __restrict__ out_b,
    int64_t* __restrict__ out_c, float* __restrict__ value, float* __restrict__ libration,
    int32_t* __restrict__ tls_rank) {
  const int sub = threadIdx.x & (BG_LANES - 1);
  const int64_t i = (int64_t)blockIdx.x * BG_ATOMS + (threadIdx.x / BG_LANES);
  int64_t p0 = 0, p1 = 0;
  if (i < N) bg_segment(nbr_ptr, i, E, p0, p1);
  const int64_t d = p1 - p0;
  if (d < 2) return;                                               // the whole group: d is the atom's
  const AtLib t = at_lib(params, rank, bg_row(atom_row, i, M));
  const int64_t first = angle_offset[i];
#pragma unroll 1
  for (int64_t c = 0; c < d - 1; c += BG_LANES) {
    const int64_t k1 = c + sub;
    const int64_t e1 = k1 < d - 1 ? adj[p0 + k1] : -1;
    if (e1 < 0 || e1 >= E) continue;
    const AtVec p = at_dir(cart_dir, e1);
    const AtVec pl = t.on ? at_librated(t, at_scaled(p, (double)cart_dist[e1])) : p;
    const int64_t a = src[e1], row = first + k1 * (2 * d - k1 - 1) / 2 - (k1 + 1);
#pragma unroll 1
    for (int64_t k2 = k1 + 1; k2 < d; ++k2) {
      const int64_t e2 = adj[p0 + k2], s = row + k2;
      if (e2 < 0 || e2 >= E || s < 0 || s >= na) continue;         // a slot outside the table is never written
      const AtVec q = at_dir(cart_dir, e2);
      out_a[s] = a;
      out_b[s] = i;
      out_c[s] = src[e2];
      value[s] = at_angle(p, q);
      libration[s] = t.on ? at_angle(pl, at_librated(t, at_scaled(q, (double)cart_dist[e2]))) : NAN;
      tls_rank[s] = t.rank;
    }
  }
}

__global__ __launch_bounds__(BG_THREADS) void cn_torsion_fill_kernel(
    const int64_t* __restrict__ src, const float* __restrict__ cart_dist, const float* __restrict__ cart_dir,
    const int64_t* __restrict__ atom_row, const int64_t* __restrict__ nbr_ptr, const int64_t* __restrict__ offset,
    const int64_t* __restrict__ adj, const int64_t* __restrict__ bond_edge, const int64_t* __restrict__ reverse,
    const int64_t* __restrict__ torsion_offset, const float* __restrict__ params, const int32_t* __restrict__ rank,
    int64_t N, int64_t M, int64_t E, int64_t nb, int64_t nt, int64_t* __restrict__ out_a, int64_t* __restrict__ out_b,
    int64_t* __restrict__ out_c, int64_t* __restrict__ out_d, float* __restrict__ value, float* __restrict__ libration,
    int32_t* __restrict__ tls_rank) {
  const int sub = threadIdx.x & (BG_LANES - 1);
  const int64_t i = (int64_t)blockIdx.x * BG_ATOMS + (threadIdx.x / BG_LANES);
  int64_t p0 = 0, p1 = 0, k0 = 0, k1 = 0;
  if (i < N) {
    bg_segment(nbr_ptr, i, E, p0, p1);
    bg_segment(offset, i, nb, k0, k1);
  }
  const int64_t nd = p1 - p0 - 1;
  if (nd < 1 || k1 <= k0) return;                                  // the whole group
  const AtLib t = at_lib(params, rank, bg_row(atom_row, i, M));
#pragma unroll 1
  for (int64_t kb = k0; kb < k1; ++kb) {                           // the listed bonds e0 = (b -> i) of this atom c = i
    const int64_t e0 = bond_edge[kb], rev = reverse[kb];
    int64_t b = (e0 >= 0 && e0 < E) ? src[e0] : -1, q0 = 0, q1 = 0;
    if (b < 0 || b >= N) continue;
    bg_segment(nbr_ptr, b, E, q0, q1);
    const int64_t n_a = (q1 - q0) - (rev >= 0 ? 1 : 0), total = n_a * nd, first = torsion_offset[kb];
    const AtVec b2 = at_dir(cart_dir, e0);
    const AtVec b2l = t.on ? at_librated(t, at_scaled(b2, (double)cart_dist[e0])) : b2;
#pragma unroll 1
    for (int64_t w = sub; w < total; w += BG_LANES) {
      const int64_t ia = w / nd, id = w - ia * nd, s = first + w;
      int64_t ea = adj[q0 + ia], ed = adj[p0 + id];
      if (rev >= 0 && ea >= rev) ea = adj[q0 + ia + 1 < q1 ? q0 + ia + 1 : q1 - 1];
      if (ed >= e0) ed = adj[p0 + id + 1 < p1 ? p0 + id + 1 : p1 - 1];
      if (ea < 0 || ea >= E || ed < 0 || ed >= E || s < 0 || s >= nt) continue;
      const AtVec b1 = at_dir(cart_dir, ea), dd = at_dir(cart_dir, ed);
      const AtVec b3 = {-dd.x, -dd.y, -dd.z};
      bool defined;
      const float v = at_torsion(b1, b2, b3, defined);
      float lib = NAN;
      if (t.on && defined) {
        const AtVec vd = at_librated(t, at_scaled(dd, (double)cart_dist[ed]));
        const AtVec b3l = {-vd.x, -vd.y, -vd.z};
        bool unused;
        lib = at_torsion(at_librated(t, at_scaled(b1, (double)cart_dist[ea])), b2l, b3l, unused);
      }
      out_a[s] = src[ea];
      out_b[s] = b;
      out_c[s] = i;
      out_d[s] = src[ed];
      value[s] = defined ? v : NAN;
      libration[s] = lib;
      tls_rank[s] = t.rank;
    }
  }
}

// angle_stats[g] = (entries, sum of value, entries with a finite libration, sum and largest of |libration - value| over
// those); torsion_stats[g] = (entries, entries with a NaN value, entries with a finite libration, sum and largest of the
// circular |libration - value| over those).  An angle belongs to the crystal of b, a torsion to that of c.
__global__ __launch_bounds__(WAVE) void cn_angle_table_crystal_kernel(
    const int64_t* __restrict__ atom_ptr, const int64_t* __restrict__ offset, const int64_t* __restrict__ angle_offset,
    const int64_t* __restrict__ torsion_offset, int64_t N, int64_t nb, int64_t na, int64_t nt,
    const float* __restrict__ angle_value, const float* __restrict__ angle_libration,
    const float* __restrict__ torsion_value, const float* __restrict__ torsion_libration,
    double* __restrict__ angle_stats, double* __restrict__ torsion_stats) {
  const int g = blockIdx.x, lane = threadIdx.x;
  int64_t a0, a1;
  cr_rows(atom_ptr, g, N, a0, a1);
  a0 = a0 > N ? N : a0;                                            // the scans have N + 1 entries
  a1 = a1 < a0 ? a0 : a1;
  int64_t s0 = angle_offset[a0], s1 = angle_offset[a1], k0 = offset[a0], k1 = offset[a1];
  s0 = s0 < 0 ? 0 : s0;
  s1 = s1 > na ? na : s1;
  k0 = k0 < 0 ? 0 : (k0 > nb ? nb : k0);                           // torsion_offset has nb + 1 entries
  k1 = k1 < k0 ? k0 : (k1 > nb ? nb : k1);
  int64_t t0 = torsion_offset[k0], t1 = torsion_offset[k1];
  t0 = t0 < 0 ? 0 : t0;
  t1 = t1 > nt ? nt : t1;
  double sum = 0.0, nl = 0.0, grow = 0.0, top = 0.0;
  for (int64_t s = s0 + lane; s < s1; s += WAVE) {
    const double v = (double)angle_value[s], lib = (double)angle_libration[s];
    sum += v;
    if (lib - lib == 0.0) {                                        // finite
      const double x = fabs(lib - v);
      nl += 1.0;
      grow += x;
      top = cr_max_nan(top, x);
    }
  }
  sum = cr_wave_sum(sum);
  nl = cr_wave_sum(nl);
  grow = cr_wave_sum(grow);
  top = cr_wave_max_nan(top);
  if (lane == 0) {
    double* __restrict__ o = angle_stats + (size_t)g * 5;
    o[0] = (double)(s1 > s0 ? s1 - s0 : 0);
    o[1] = sum;
    o[2] = nl;
    o[3] = grow;
    o[4] = top;
  }
  double bad = 0.0;
  nl = 0.0, grow = 0.0, top = 0.0;
  for (int64_t s = t0 + lane; s < t1; s += WAVE) {
    const double v = (double)torsion_value[s], lib = (double)torsion_libration[s];
    bad += v != v ? 1.0 : 0.0;
    if (lib - lib == 0.0) {
      double x = fabs(lib - v);
      x = 360.0 - x < x ? 360.0 - x : x;
      nl += 1.0;
      grow += x;
      top = cr_max_nan(top, x);
    }
  }
  bad = cr_wave_sum(bad);
  nl = cr_wave_sum(nl);
  grow = cr_wave_sum(grow);
  top = cr_wave_max_nan(top);
  if (lane == 0) {
    double* __restrict__ o = torsion_stats + (size_t)g * 5;
    o[0] = (double)(t1 > t0 ? t1 - t0 : 0);
    o[1] = bad;
    o[2] = nl;
    o[3] = grow;
    o[4] = top;
  }
}

constexpr int64_t AT_MAX_ATOMS = (1LL << 31) * BG_ATOMS;

inline dim3 at_grid(int64_t N) { return dim3((unsigned)((N + BG_ATOMS - 1) / BG_ATOMS)); }

}  // namespace

extern "C" int cartnet_bond_adjacency(const int64_t* z, const int64_t* edge_index, const float* cart_dist,
                                      const int64_t* atom_row, const int64_t* seg_ptr, const float* radii, int32_t n_radii,
                                      float tol, const int64_t* nbr_ptr, const int64_t* offset, int64_t N, int64_t M,
                                      int64_t E, int64_t nb, int64_t* adj, int64_t* bond_edge, void* stream) {
  CN_CHECK(N >= 0 && M >= 0 && E >= 0 && nb >= 0 && n_radii >= 0, "cartnet_bond_adjacency: bad sizes (N=%lld, M=%lld, "
           "E=%lld, nb=%lld, n_radii=%d)", (long long)N, (long long)M, (long long)E, (long long)nb, n_radii);
  CN_CHECK(tol == tol, "cartnet_bond_adjacency: tol must be a number");
  CN_CHECK(N < AT_MAX_ATOMS, "cartnet_bond_adjacency: too many atoms for one launch");
  if (N == 0 || E == 0) return 0;                                  // without edges no list has an entry
  CN_CHECK(z && edge_index && cart_dist && atom_row && seg_ptr && radii && nbr_ptr && offset && adj,
           "cartnet_bond_adjacency: null pointer");
  CN_CHECK(nb == 0 || bond_edge, "cartnet_bond_adjacency: null pointer (%lld listed bonds need bond_edge)", (long long)nb);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cn_bond_adjacency_kernel, at_grid(N), dim3(BG_THREADS), 0, st, z, edge_index, cart_dist, atom_row,
                     seg_ptr, radii, (int)n_radii, tol, nbr_ptr, offset, N, M, E, nb, adj, bond_edge);
  CN_LAUNCH_CHECK("cartnet_bond_adjacency");
  return 0;
}

extern "C" int cartnet_angle_table_count(const int64_t* edge_index, const float* cart_dist, const float* cart_dir,
                                         const int64_t* nbr_ptr, const int64_t* offset, const int64_t* adj,
                                         const int64_t* bond_edge, int64_t N, int64_t E, int64_t nb, int64_t* angle_count,
                                         int64_t* reverse, int64_t* torsion_count, void* stream) {
  CN_CHECK(N >= 0 && E >= 0 && nb >= 0, "cartnet_angle_table_count: bad sizes (N=%lld, E=%lld, nb=%lld)", (long long)N,
           (long long)E, (long long)nb);
  CN_CHECK(N < AT_MAX_ATOMS, "cartnet_angle_table_count: too many atoms for one launch");
  if (N == 0) return 0;
  CN_CHECK(nbr_ptr && offset && angle_count, "cartnet_angle_table_count: null pointer");
  CN_CHECK(E == 0 || (edge_index && cart_dist && cart_dir && adj), "cartnet_angle_table_count: null pointer");
  CN_CHECK(nb == 0 || (E > 0 && bond_edge && reverse && torsion_count),
           "cartnet_angle_table_count: null pointer (%lld listed bonds need the edges and both per-bond outputs)",
           (long long)nb);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // without edges every range is empty: the atoms get their zeros from the same launch
  hipLaunchKernelGGL(cn_angle_count_kernel, at_grid(N), dim3(BG_THREADS), 0, st, edge_index, cart_dist, cart_dir, nbr_ptr,
                     offset, adj, bond_edge, N, E, nb, angle_count, reverse, torsion_count);
  CN_LAUNCH_CHECK("cartnet_angle_table_count");
  return 0;
}

extern "C" int cartnet_adp_angle_table(const int64_t* edge_index, const float* cart_dist, const float* cart_dir,
                                       const int64_t* atom_row, const int64_t* atom_ptr, const int64_t* nbr_ptr,
                                       const int64_t* offset, const int64_t* adj, const int64_t* bond_edge,
                                       const int64_t* reverse, const int64_t* angle_offset, const int64_t* torsion_offset,
                                       const float* params, const int32_t* rank, int32_t B, int64_t N, int64_t M, int64_t E,
                                       int64_t nb, int64_t na, int64_t nt, int64_t* angle_a, int64_t* angle_b,
                                       int64_t* angle_c, float* angle_value, float* angle_libration,
                                       int32_t* angle_tls_rank, int64_t* torsion_a, int64_t* torsion_b, int64_t* torsion_c,
                                       int64_t* torsion_d, float* torsion_value, float* torsion_libration,
                                       int32_t* torsion_tls_rank, double* angle_stats, double* torsion_stats,
                                       void* stream) {
  CN_CHECK(B >= 0 && N >= 0 && M >= 0 && E >= 0 && nb >= 0 && na >= 0 && nt >= 0,
           "cartnet_adp_angle_table: bad sizes (B=%d, N=%lld, M=%lld, E=%lld, nb=%lld, na=%lld, nt=%lld)", B, (long long)N,
           (long long)M, (long long)E, (long long)nb, (long long)na, (long long)nt);
  CN_CHECK(N < AT_MAX_ATOMS, "cartnet_adp_angle_table: too many atoms for one launch");
  CN_CHECK((params == nullptr) == (rank == nullptr), "cartnet_adp_angle_table: params and rank come together or not at all");
  CN_CHECK((angle_stats == nullptr) == (torsion_stats == nullptr),
           "cartnet_adp_angle_table: the two statistics come together or not at all");
  if (B == 0 || N == 0) return 0;
  CN_CHECK(atom_row && atom_ptr && nbr_ptr && offset && angle_offset && torsion_offset,
           "cartnet_adp_angle_table: null pointer");
  CN_CHECK(na == 0 || (edge_index && cart_dist && cart_dir && adj && angle_a && angle_b && angle_c && angle_value &&
                       angle_libration && angle_tls_rank && M > 0 && E > 0),
           "cartnet_adp_angle_table: null pointer (%lld angles need the edges, the adjacency and every output)",
           (long long)na);
  CN_CHECK(nt == 0 || (edge_index && cart_dist && cart_dir && adj && bond_edge && reverse && torsion_a && torsion_b &&
                       torsion_c && torsion_d && torsion_value && torsion_libration && torsion_tls_rank && M > 0 &&
                       E > 0 && nb > 0),
           "cartnet_adp_angle_table: null pointer (%lld torsions need the edges, the lists and every output)",
           (long long)nt);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (na > 0) {
    hipLaunchKernelGGL(cn_angle_fill_kernel, at_grid(N), dim3(BG_THREADS), 0, st, edge_index, cart_dist, cart_dir,
                       atom_row, nbr_ptr, adj, angle_offset, params, rank, N, M, E, na, angle_a, angle_b, angle_c,
                       angle_value, angle_libration, angle_tls_rank);
    CN_LAUNCH_CHECK("cartnet_adp_angle_table");
  }
  if (nt > 0) {
    hipLaunchKernelGGL(cn_torsion_fill_kernel, at_grid(N), dim3(BG_THREADS), 0, st, edge_index, cart_dist, cart_dir,
                       atom_row, nbr_ptr, offset, adj, bond_edge, reverse, torsion_offset, params, rank, N, M, E, nb, nt,
                       torsion_a, torsion_b, torsion_c, torsion_d, torsion_value, torsion_libration, torsion_tls_rank);
    CN_LAUNCH_CHECK("cartnet_adp_angle_table");
  }
  if (angle_stats) {
    hipLaunchKernelGGL(cn_angle_table_crystal_kernel, dim3(B), dim3(WAVE), 0, st, atom_ptr, offset, angle_offset,
                       torsion_offset, N, nb, na, nt, angle_value, angle_libration, torsion_value, torsion_libration,
                       angle_stats, torsion_stats);
    CN_LAUNCH_CHECK("cartnet_adp_angle_table");
  }
  return 0;
}

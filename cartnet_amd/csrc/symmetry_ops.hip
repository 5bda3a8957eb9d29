// From the asymmetric unit of a CIF to the contents of the unit cell, and back (cartnet_amd/symmetry.py).
//
// Reference: dataset/extract_csd_data.py:84-123 asks the CSD API for the packed cell (crystal.packing), drops repeated
// atoms on the host (delete_repeated, :28-40: an all-pairs distance matrix per crystal) and brings the file's U_ij into
// the Cartesian frame (:115-123).  Here the symmetry operators of the file generate the candidates and the same rule
// runs over all crystals of a call at once.  Candidate c = s * n + a of a crystal with n atoms and m operators is atom a
// under operator s (operator 0 is the identity: the asymmetric unit comes first).  A workgroup owns a tile of 256
// consecutive candidates of ONE crystal (a tile table from the host: crystal and first candidate per tile).
//
//   count:  cn_sy_candidates  f' = ((W0 f0 + W1 f1) + W2 f2) + w in fp64 (W in {-1, 0, 1}: the products are exact),
//                             minus floor, rounded to fp32, then delete_repeated's normalisation (:29-31); 16-byte rows.
//                             Also status[g][0] = the cell is singular or not finite.
//           cn_sy_first_dup   rep[i] = the lowest j < i of the crystal closer than 1e-4 (fp32, no periodic wrap), else i:
//                             the earlier candidates pass through LDS in tiles of 256, every lane reads the same slot
//                             per step (a broadcast).  i is kept iff rep[i] == i: mask_to_keep of :32-40.
//           cn_sy_count       kept atoms and kept non-hydrogen atoms per tile; status[g][1] = some rep[rep[i]] != rep[i]
//                             (atoms between one and two thresholds apart: the rule is not transitive there)
//           cn_sy_scan        one workgroup: so_tile_scan of both sums, the status words folded into totals
//           cn_sy_rank        scan inside the tile + the tile's carry -> rank_a / rank_h (-1 = dropped), atom_ptr', y_ptr'
//   fill:   cn_sy_fill        z, pos (normalised fraction times cell in fp64, rounded once), non_h_mask, row_asym / row_op
//                             per non-hydrogen row, orbit_row per (non-hydrogen asymmetric atom, operator), cell as fp32
//   cn_sy_targets   per row: y = cell^T (W (N U_cif N) W^T) cell in fp64, stored as fp32 (:115-123 plus the operator)
//   cn_sy_average   per non-hydrogen asymmetric atom of a batch: the mean over the operators of the predictions of its
//                   orbit, each brought back to the site, as U_cif; and their largest deviation from that mean
//
// Reduce-then-scan as in shard_ops.hip: no workgroup waits for another, no atomics, every output position is a pure
// function of the input, so two runs give the same bytes.  Compiled with -ffp-contract=off: the operation order above is
// the rule (cartnet_amd.symmetry.expand_host states it in torch).
#include "common.h"
#include "shard_tiles.h"

#include <math.h>

namespace {

constexpr int SY_T = SO_THREADS;                 // candidates per tile

struct SyIn {
  const int64_t* asym_ptr;
  const double* asym_frac;
  const int32_t* asym_z;
  const int64_t* op_ptr;
  const int8_t* op_rot;
  const double* op_trans;
  const double* cell;
  const int64_t* cand_ptr;
  const int32_t* tile_g;
  const int64_t* tile_c0;
  int G;
  int64_t A, S, C;
};

// the candidate of this thread: crystal g, its candidates [base, end), candidate i = atom a under operator s
struct SyItem {
  int g, n, m, a, s;
  int64_t base, end, c0, i;
  bool valid;
};

// False (for the whole workgroup) if the tile table or the offsets are inconsistent: nothing is then read or written
__device__ __forceinline__ bool sy_item(const SyIn& p, SyItem& it) {
  it.g = p.tile_g[blockIdx.x];
  it.c0 = p.tile_c0[blockIdx.x];
  if (it.g < 0 || it.g >= p.G) return false;
  it.base = p.cand_ptr[it.g];
  it.end = p.cand_ptr[it.g + 1];
  const int64_t a0 = p.asym_ptr[it.g], a1 = p.asym_ptr[it.g + 1], s0 = p.op_ptr[it.g], s1 = p.op_ptr[it.g + 1];
  if (a0 < 0 || a1 > p.A || a1 <= a0 || s0 < 0 || s1 > p.S || s1 <= s0) return false;
  if (a1 - a0 >= (1LL << 31) || s1 - s0 >= (1LL << 31)) return false;
  it.n = (int)(a1 - a0);
  it.m = (int)(s1 - s0);
  if (it.base < 0 || it.end > p.C || it.end - it.base != (int64_t)it.n * it.m) return false;
  if (it.c0 < it.base || it.c0 >= it.end || (it.c0 - it.base) % SY_T != 0) return false;
  it.i = it.c0 + threadIdx.x;
  it.valid = it.i < it.end;
  const int64_t lc = it.i - it.base;
  it.s = it.valid ? (int)(lc / it.n) : 0;
  it.a = it.valid ? (int)(lc % it.n) : 0;
  return true;
}

// delete_repeated's normalisation (:29-31) of one fp32 coordinate
__device__ __forceinline__ float sy_normalise(float x) {
  if (x < 0.f) x = x + 1.f;
  if (x > 1.f) x = x - 1.f;
  if (fabsf(x - 1.f) <= 1e-4f + 1e-5f) x = 0.f;            // isclose(x, 1, atol=1e-4) with torch's default rtol=1e-5
  return x;
}

// The reciprocal vectors r[i][.] = a*, b*, c* of the fp64 cell whose rows are the lattice vectors (the rows of
// inv(cell^T)) and their lengths; false if det == 0 or anything is not finite.
__device__ __forceinline__ bool sy_reciprocal(const double* __restrict__ cell, double r[3][3], double len[3]) {
  double a[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) a[i][j] = cell[i * 3 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int p = (i + 1) % 3, q = (i + 2) % 3;
    r[i][0] = a[p][1] * a[q][2] - a[p][2] * a[q][1];
    r[i][1] = a[p][2] * a[q][0] - a[p][0] * a[q][2];
    r[i][2] = a[p][0] * a[q][1] - a[p][1] * a[q][0];
  }
  const double det = a[0][0] * r[0][0] + a[0][1] * r[0][1] + a[0][2] * r[0][2];
  bool ok = det != 0.0 && isfinite(det);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      ok = ok && isfinite(a[i][j]);
      r[i][j] = r[i][j] / det;
    }
    len[i] = sqrt(r[i][0] * r[i][0] + r[i][1] * r[i][1] + r[i][2] * r[i][2]);
  }
  return ok;
}

// out = L in L^T for an integer 3x3 L (row-major) and a symmetric fp64 matrix
__device__ __forceinline__ void sy_conjugate(const int L[9], const double in[3][3], double out[3][3]) {
  double t[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      t[i][j] = ((double)L[i * 3] * in[0][j] + (double)L[i * 3 + 1] * in[1][j]) + (double)L[i * 3 + 2] * in[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      out[i][j] = (t[i][0] * (double)L[j * 3] + t[i][1] * (double)L[j * 3 + 1]) + t[i][2] * (double)L[j * 3 + 2];
}

__global__ __launch_bounds__(SY_T) void cn_sy_candidates(SyIn p, f32x4* __restrict__ coord,
                                                         int32_t* __restrict__ status) {
  SyItem it;
  if (!sy_item(p, it)) return;
  if (it.i == it.base) {
    double r[3][3], len[3];
    status[2 * it.g] = sy_reciprocal(p.cell + (size_t)it.g * 9, r, len) ? 0 : 1;
  }
  if (!it.valid) return;
  const double* __restrict__ f = p.asym_frac + (p.asym_ptr[it.g] + it.a) * 3;
  const int8_t* __restrict__ W = p.op_rot + (p.op_ptr[it.g] + it.s) * 9;
  const double* __restrict__ w = p.op_trans + (p.op_ptr[it.g] + it.s) * 3;
  const double f0 = f[0], f1 = f[1], f2 = f[2];
  float x[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double v = (((double)W[k * 3] * f0 + (double)W[k * 3 + 1] * f1) + (double)W[k * 3 + 2] * f2) + w[k];
    v = v - floor(v);
    x[k] = sy_normalise((float)v);
  }
  f32x4 o;
  o.x = x[0]; o.y = x[1]; o.z = x[2]; o.w = 0.f;
  coord[it.i] = o;
}

__global__ __launch_bounds__(SY_T) void cn_sy_first_dup(SyIn p, const f32x4* __restrict__ coord,
                                                        int64_t* __restrict__ rep) {
  __shared__ f32x4 tile[SY_T];
  SyItem it;
  if (!sy_item(p, it)) return;                               // workgroup-uniform
  f32x4 me;
  me.x = me.y = me.z = me.w = 0.f;
  if (it.valid) me = coord[it.i];
  int64_t r = it.i;
  for (int64_t j0 = it.base; j0 <= it.c0; j0 += SY_T) {      // uniform bounds: every thread reaches every barrier
    const int64_t jj = j0 + threadIdx.x;
    f32x4 t;
    t.x = t.y = t.z = t.w = 0.f;
    if (jj < it.end) t = coord[jj];
    tile[threadIdx.x] = t;
    __syncthreads();
    const int64_t lim = it.i - j0;                           // only candidates before i
#pragma unroll 8
    for (int k = 0; k < SY_T; ++k) {
      const f32x4 o = tile[k];
      const float dx = me.x - o.x, dy = me.y - o.y, dz = me.z - o.z;
      const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
      if (k < lim && r == it.i && d < 1e-4f) r = j0 + k;
    }
    __syncthreads();
  }
  if (it.valid) rep[it.i] = r;
}

// kept / kept and not hydrogen, for this thread's candidate
__device__ __forceinline__ void sy_flags(const SyIn& p, const SyItem& it, const int64_t* __restrict__ rep, int& keep,
                                         int& heavy) {
  keep = it.valid && rep[it.i] == it.i;
  heavy = keep && p.asym_z[p.asym_ptr[it.g] + it.a] != 1;
}

__global__ __launch_bounds__(SY_T) void cn_sy_count(SyIn p, const int64_t* __restrict__ rep,
                                                    int32_t* __restrict__ sum_a, int32_t* __restrict__ sum_h,
                                                    int32_t* __restrict__ status) {
  __shared__ int lds[SY_T / WAVE];
  SyItem it;
  if (!sy_item(p, it)) {
    if (threadIdx.x == 0) sum_a[blockIdx.x] = sum_h[blockIdx.x] = 0;
    return;
  }
  int keep, heavy;
  sy_flags(p, it, rep, keep, heavy);
  if (it.valid) {
    const int64_t r = rep[it.i];
    if (rep[r] != r) status[2 * it.g + 1] = 1;               // every writer stores the same word
  }
  int ta, th;
  so_block_scan(keep, lds, ta);
  so_block_scan(heavy, lds, th);
  if (threadIdx.x == 0) {
    sum_a[blockIdx.x] = ta;
    sum_h[blockIdx.x] = th;
  }
}

__global__ __launch_bounds__(SY_T) void cn_sy_scan(const int32_t* __restrict__ sum_a, const int32_t* __restrict__ sum_h,
                                                   int64_t nT, int64_t* __restrict__ off_a, int64_t* __restrict__ off_h,
                                                   const int32_t* __restrict__ status, int G,
                                                   int64_t* __restrict__ totals, int64_t* __restrict__ atom_ptr_out,
                                                   int64_t* __restrict__ y_ptr_out) {
  __shared__ int64_t lds[SY_T / WAVE];
  __shared__ int64_t fold[2 * (SY_T / WAVE)];
  so_tile_scan(sum_a, nT, off_a, totals, lds);
  so_tile_scan(sum_h, nT, off_h, totals + 1, lds);
  int64_t bits = 0, first = G;
  for (int g = threadIdx.x; g < G; g += SY_T) {
    const int64_t b = (status[2 * g] ? 1 : 0) | (status[2 * g + 1] ? 2 : 0);
    bits |= b;
    if (b && g < first) first = g;
  }
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    bits |= __shfl_xor(bits, o);
    const int64_t f = __shfl_xor(first, o);
    first = f < first ? f : first;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    fold[threadIdx.x >> 6] = bits;
    fold[SY_T / WAVE + (threadIdx.x >> 6)] = first;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < SY_T / WAVE; ++w) {
      bits |= fold[w];
      first = fold[SY_T / WAVE + w] < first ? fold[SY_T / WAVE + w] : first;
    }
    totals[2] = bits;
    totals[3] = bits ? first : -1;
    atom_ptr_out[G] = off_a[nT];                              // this thread wrote both
    y_ptr_out[G] = off_h[nT];
  }
}

__global__ __launch_bounds__(SY_T) void cn_sy_rank(SyIn p, const int64_t* __restrict__ rep,
                                                   const int64_t* __restrict__ off_a, const int64_t* __restrict__ off_h,
                                                   int64_t* __restrict__ rank_a, int64_t* __restrict__ rank_h,
                                                   int64_t* __restrict__ atom_ptr_out, int64_t* __restrict__ y_ptr_out) {
  __shared__ int lds[SY_T / WAVE];
  SyItem it;
  if (!sy_item(p, it)) return;
  int keep, heavy, tot;
  sy_flags(p, it, rep, keep, heavy);
  const int64_t ra = off_a[blockIdx.x] + so_block_scan(keep, lds, tot);
  const int64_t rh = off_h[blockIdx.x] + so_block_scan(heavy, lds, tot);
  if (!it.valid) return;
  if (it.i == it.base) {                                     // a crystal has at least one candidate
    atom_ptr_out[it.g] = ra;
    y_ptr_out[it.g] = rh;
  }
  rank_a[it.i] = keep ? ra : -1;
  rank_h[it.i] = heavy ? rh : -1;
}

struct SyOut {
  int32_t* z;
  float* pos;
  uint8_t* mask;
  int32_t* row_asym;
  int32_t* row_op;
  int32_t* orbit_row;
  float* cell;
};

__global__ __launch_bounds__(SY_T) void cn_sy_fill(SyIn p, const f32x4* __restrict__ coord,
                                                   const int64_t* __restrict__ rep, const int64_t* __restrict__ rank_a,
                                                   const int64_t* __restrict__ rank_h,
                                                   const int64_t* __restrict__ y_ptr_out,
                                                   const int32_t* __restrict__ asym_site,
                                                   const int64_t* __restrict__ orb_ptr, int64_t N_out, int64_t Y_out,
                                                   SyOut o) {
  SyItem it;
  if (!sy_item(p, it) || !it.valid) return;
  const double* __restrict__ cell = p.cell + (size_t)it.g * 9;
  if (it.i == it.base)
    for (int k = 0; k < 9; ++k) o.cell[(size_t)it.g * 9 + k] = (float)cell[k];
  const int z = p.asym_z[p.asym_ptr[it.g] + it.a];
  const int64_t ra = rank_a[it.i], rh = rank_h[it.i];
  if (ra >= 0 && ra < N_out) {
    const f32x4 c = coord[it.i];
    const double f0 = (double)c.x, f1 = (double)c.y, f2 = (double)c.z;
    o.z[ra] = z;
    o.mask[ra] = z != 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) o.pos[ra * 3 + k] = (float)((f0 * cell[k] + f1 * cell[3 + k]) + f2 * cell[6 + k]);
  }
  if (rh >= 0 && rh < Y_out) {
    o.row_asym[rh] = it.a;
    o.row_op[rh] = it.s;
  }
  if (z != 1) {
    const int64_t site = asym_site[p.asym_ptr[it.g] + it.a];
    const int64_t slot = orb_ptr[it.g] + site * it.m + it.s;
    if (site >= 0 && slot < orb_ptr[it.g + 1]) {
      const int64_t rr = rank_h[rep[it.i]];
      o.orbit_row[slot] = rr >= 0 ? (int32_t)(rr - y_ptr_out[it.g]) : -1;
    }
  }
}

__global__ __launch_bounds__(SY_T) void cn_sy_targets(const int64_t* __restrict__ asym_ptr,
                                                      const double* __restrict__ asym_ucif,
                                                      const int64_t* __restrict__ op_ptr,
                                                      const int8_t* __restrict__ op_rot, const double* __restrict__ cell,
                                                      const int64_t* __restrict__ y_ptr, const int32_t* __restrict__ row_asym,
                                                      const int32_t* __restrict__ row_op, int G, int64_t Y,
                                                      float* __restrict__ y) {
  const int64_t h = (int64_t)blockIdx.x * SY_T + threadIdx.x;
  if (h >= Y) return;
  const int g = so_find(y_ptr, 0, G + 1, h);
  if (g >= G) return;
  const int a = row_asym[h], s = row_op[h];
  const double nanv = (double)NAN;
  const bool in = a >= 0 && a < asym_ptr[g + 1] - asym_ptr[g] && s >= 0 && s < op_ptr[g + 1] - op_ptr[g];
  const double* __restrict__ M = cell + (size_t)g * 9;
  double r[3][3], len[3];
  const bool ok = sy_reciprocal(M, r, len) && in;
  const double* __restrict__ u = asym_ucif + (asym_ptr[g] + (in ? a : 0)) * 6;
  const int8_t* __restrict__ Wp = op_rot + (op_ptr[g] + (in ? s : 0)) * 9;
  int W[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) W[k] = Wp[k];
  // U11 U22 U33 U23 U13 U12 -> beta = N U N
  const double full[3][3] = {{u[0], u[5], u[4]}, {u[5], u[1], u[3]}, {u[4], u[3], u[2]}};
  double beta[3][3], bw[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) beta[i][j] = (len[i] * full[i][j]) * len[j];
  sy_conjugate(W, beta, bw);
  // y = cell^T beta' cell
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double t = (bw[i][0] * M[l] + bw[i][1] * M[3 + l]) + bw[i][2] * M[6 + l];
        acc += M[i * 3 + k] * t;
      }
      y[h * 9 + k * 3 + l] = (float)(ok ? acc : nanv);
    }
}

// beta at the site of asymmetric atom `site` from member s of its orbit: W^-1 (cell^-T U cell^-1) W^-T; false if the row
// is missing
__device__ __forceinline__ bool sy_member(const float* __restrict__ pred, int64_t r0, int64_t r1, int32_t orow,
                                          const int8_t* __restrict__ Wp, const double r[3][3], double out[3][3]) {
  const int64_t row = r0 + orow;
  if (orow < 0 || row >= r1) return false;
  const float* __restrict__ up = pred + row * 9;
  double u[3][3], t[3][3], b[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) u[a][c] = 0.5 * ((double)up[a * 3 + c] + (double)up[c * 3 + a]);
#pragma unroll
  for (int j = 0; j < 3; ++j)                                 // t[j] = U a*_j
#pragma unroll
    for (int a = 0; a < 3; ++a) t[j][a] = (u[a][0] * r[j][0] + u[a][1] * r[j][1]) + u[a][2] * r[j][2];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) b[i][j] = (r[i][0] * t[j][0] + r[i][1] * t[j][1]) + r[i][2] * t[j][2];
  int W[9], L[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) W[k] = Wp[k];
  const int det = W[0] * (W[4] * W[8] - W[5] * W[7]) - W[1] * (W[3] * W[8] - W[5] * W[6]) + W[2] * (W[3] * W[7] - W[4] * W[6]);
  // inverse = adjugate * det for det = +-1
  L[0] = (W[4] * W[8] - W[5] * W[7]) * det; L[1] = (W[2] * W[7] - W[1] * W[8]) * det; L[2] = (W[1] * W[5] - W[2] * W[4]) * det;
  L[3] = (W[5] * W[6] - W[3] * W[8]) * det; L[4] = (W[0] * W[8] - W[2] * W[6]) * det; L[5] = (W[2] * W[3] - W[0] * W[5]) * det;
  L[6] = (W[3] * W[7] - W[4] * W[6]) * det; L[7] = (W[1] * W[6] - W[0] * W[7]) * det; L[8] = (W[0] * W[4] - W[1] * W[3]) * det;
  sy_conjugate(L, b, out);
  return true;
}

__global__ __launch_bounds__(SY_T) void cn_sy_average(const float* __restrict__ pred, const int64_t* __restrict__ row_ptr,
                                                      const int64_t* __restrict__ sel,
                                                      const int64_t* __restrict__ bsite_ptr, int B, int64_t M, int64_t Hb,
                                                      const int64_t* __restrict__ op_ptr,
                                                      const int8_t* __restrict__ op_rot,
                                                      const int64_t* __restrict__ orb_ptr,
                                                      const int32_t* __restrict__ orbit_row,
                                                      const double* __restrict__ cell, int G, int64_t S, int64_t O,
                                                      float* __restrict__ u_cif, float* __restrict__ spread) {
  const int64_t q = (int64_t)blockIdx.x * SY_T + threadIdx.x;
  if (q >= Hb) return;
  const float nanf_ = NAN;
  const int b = so_find(bsite_ptr, 0, B + 1, q);
  const int64_t g = b < B ? sel[b] : -1;
  bool ok = g >= 0 && g < G;
  int64_t m = 0, slot = 0, r0 = 0, r1 = 0;
  if (ok) {
    const int64_t site = q - bsite_ptr[b];
    m = op_ptr[g + 1] - op_ptr[g];
    slot = orb_ptr[g] + site * m;
    r0 = row_ptr[b];
    r1 = row_ptr[b + 1] < M ? row_ptr[b + 1] : M;
    ok = m > 0 && op_ptr[g] >= 0 && op_ptr[g + 1] <= S && slot >= 0 && slot + m <= orb_ptr[g + 1] && orb_ptr[g + 1] <= O &&
         r0 >= 0;
  }
  double r[3][3], len[3];
  ok = ok && sy_reciprocal(cell + (size_t)(ok ? g : 0) * 9, r, len);
  double mean[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (ok) {
#pragma unroll 1
    for (int64_t s = 0; s < m; ++s) {
      double mem[3][3];
      ok = ok && sy_member(pred, r0, r1, orbit_row[slot + s], op_rot + (op_ptr[g] + s) * 9, r, mem);
      if (!ok) break;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) mean[i][j] += mem[i][j];
    }
  }
  double dev = 0.0;
  if (ok) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) mean[i][j] = mean[i][j] / (double)m;
#pragma unroll 1
    for (int64_t s = 0; s < m; ++s) {
      double mem[3][3];
      sy_member(pred, r0, r1, orbit_row[slot + s], op_rot + (op_ptr[g] + s) * 9, r, mem);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) dev = fmax(dev, fabs(mem[i][j] - mean[i][j]) / (len[i] * len[j]));
    }
  }
  const int ci[6] = {0, 1, 2, 1, 0, 0}, cj[6] = {0, 1, 2, 2, 2, 1};
#pragma unroll
  for (int k = 0; k < 6; ++k) u_cif[q * 6 + k] = ok ? (float)(mean[ci[k]][cj[k]] / (len[ci[k]] * len[cj[k]])) : nanf_;
  spread[q] = ok ? (float)dev : nanf_;
}

struct SyLayout {
  size_t coord, rep, rank_a, rank_h, sum_a, sum_h, off_a, off_h, status, bytes;
};

inline size_t sy_align(size_t b) { return (b + 255) / 256 * 256; }

SyLayout sy_layout(int32_t G, int64_t C, int64_t nT) {
  SyLayout l;
  size_t o = 0;
  l.coord = o;  o += sy_align((size_t)C * 16);
  l.rep = o;    o += sy_align((size_t)C * 8);
  l.rank_a = o; o += sy_align((size_t)C * 8);
  l.rank_h = o; o += sy_align((size_t)C * 8);
  l.sum_a = o;  o += sy_align((size_t)nT * 4);
  l.sum_h = o;  o += sy_align((size_t)nT * 4);
  l.off_a = o;  o += sy_align((size_t)(nT + 1) * 8);
  l.off_h = o;  o += sy_align((size_t)(nT + 1) * 8);
  l.status = o; o += sy_align((size_t)G * 8);
  l.bytes = o;
  return l;
}

#define ST(s) reinterpret_cast<hipStream_t>(s)

int sy_check(const SyIn& in, int64_t n_tiles, const void* ws, size_t ws_bytes, const char* who) {
  CN_CHECK(in.G >= 1 && in.A >= 1 && in.S >= 1 && in.C >= 1 && n_tiles >= 1, "%s: bad sizes (G=%d)", who, in.G);
  CN_CHECK(in.C < (1LL << 40) && n_tiles < (1LL << 31), "%s: too many candidates for one launch", who);
  CN_CHECK(n_tiles * (int64_t)SY_T >= in.C, "%s: the tile table does not cover the candidates", who);
  CN_CHECK(in.asym_ptr && in.asym_frac && in.asym_z && in.op_ptr && in.op_rot && in.op_trans && in.cell && in.cand_ptr &&
           in.tile_g && in.tile_c0, "%s: null array", who);
  CN_CHECK(ws && ws_bytes >= sy_layout(in.G, in.C, n_tiles).bytes, "%s: workspace too small", who);
  CN_CHECK(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "%s: workspace must be 16-byte aligned", who);
  return 0;
}

// the inputs of count and fill: ten arrays, then G, A, S, C and the number of tiles
#define SY_ARGS                                                                                                         \
  const int64_t* asym_ptr, const double* asym_frac, const int32_t* asym_z, const int64_t* op_ptr, const int8_t* op_rot, \
      const double* op_trans, const double* cell, const int64_t* cand_ptr, const int32_t* tile_crystal,                 \
      const int64_t* tile_start, int32_t G, int64_t A, int64_t S, int64_t C, int64_t n_tiles
#define SY_IN \
  SyIn { asym_ptr, asym_frac, asym_z, op_ptr, op_rot, op_trans, cell, cand_ptr, tile_crystal, tile_start, G, A, S, C }

}  // namespace

extern "C" size_t cartnet_symmetry_expand_workspace_bytes(int32_t G, int64_t C, int64_t n_tiles) {
  if (G < 0 || C < 0 || n_tiles < 0) return 0;
  return sy_layout(G, C, n_tiles).bytes;
}

extern "C" int cartnet_symmetry_expand_count(SY_ARGS, void* workspace, size_t workspace_bytes,
                                             int64_t* atom_ptr_out, int64_t* y_ptr_out, int64_t* totals, void* stream) {
  const SyIn p = SY_IN;
  if (sy_check(p, n_tiles, workspace, workspace_bytes, "cartnet_symmetry_expand_count")) return 1;
  CN_CHECK(atom_ptr_out && y_ptr_out && totals, "cartnet_symmetry_expand_count: null output");
  const SyLayout l = sy_layout(G, C, n_tiles);
  char* ws = static_cast<char*>(workspace);
  f32x4* coord = reinterpret_cast<f32x4*>(ws + l.coord);
  int64_t* rep = reinterpret_cast<int64_t*>(ws + l.rep);
  int64_t* rank_a = reinterpret_cast<int64_t*>(ws + l.rank_a);
  int64_t* rank_h = reinterpret_cast<int64_t*>(ws + l.rank_h);
  int32_t* sum_a = reinterpret_cast<int32_t*>(ws + l.sum_a);
  int32_t* sum_h = reinterpret_cast<int32_t*>(ws + l.sum_h);
  int64_t* off_a = reinterpret_cast<int64_t*>(ws + l.off_a);
  int64_t* off_h = reinterpret_cast<int64_t*>(ws + l.off_h);
  int32_t* status = reinterpret_cast<int32_t*>(ws + l.status);
  const dim3 grid((unsigned)n_tiles), block(SY_T);
  if (hipMemsetAsync(status, 0, (size_t)G * 8, ST(stream)) != hipSuccess) {
    cartnet_set_error("cartnet_symmetry_expand_count: hipMemsetAsync failed");
    return 2;
  }
  hipLaunchKernelGGL(cn_sy_candidates, grid, block, 0, ST(stream), p, coord, status);
  CN_LAUNCH_CHECK("cartnet_symmetry_expand_count/candidates");
  hipLaunchKernelGGL(cn_sy_first_dup, grid, block, 0, ST(stream), p, coord, rep);
  CN_LAUNCH_CHECK("cartnet_symmetry_expand_count/first_dup");
  hipLaunchKernelGGL(cn_sy_count, grid, block, 0, ST(stream), p, rep, sum_a, sum_h, status);
  CN_LAUNCH_CHECK("cartnet_symmetry_expand_count/count");
  hipLaunchKernelGGL(cn_sy_scan, dim3(1), block, 0, ST(stream), sum_a, sum_h, n_tiles, off_a, off_h, status, G,
                     totals, atom_ptr_out, y_ptr_out);
  CN_LAUNCH_CHECK("cartnet_symmetry_expand_count/scan");
  hipLaunchKernelGGL(cn_sy_rank, grid, block, 0, ST(stream), p, rep, off_a, off_h, rank_a, rank_h, atom_ptr_out,
                     y_ptr_out);
  CN_LAUNCH_CHECK("cartnet_symmetry_expand_count/rank");
  return 0;
}

extern "C" int cartnet_symmetry_expand_fill(SY_ARGS, const void* workspace, size_t workspace_bytes,
                                            const int64_t* y_ptr_out, const int32_t* asym_site, const int64_t* orb_ptr,
                                            int64_t N_out, int64_t Y_out, int32_t* z_out, float* pos_out,
                                            uint8_t* non_h_mask_out, int32_t* row_asym, int32_t* row_op,
                                            int32_t* orbit_row, float* cell_out, void* stream) {
  const SyIn p = SY_IN;
  if (sy_check(p, n_tiles, workspace, workspace_bytes, "cartnet_symmetry_expand_fill")) return 1;
  CN_CHECK(N_out >= 0 && N_out <= C && Y_out >= 0 && Y_out <= N_out, "cartnet_symmetry_expand_fill: bad totals");
  CN_CHECK(y_ptr_out && asym_site && orb_ptr && cell_out, "cartnet_symmetry_expand_fill: null array");
  CN_CHECK(N_out == 0 || (z_out && pos_out && non_h_mask_out), "cartnet_symmetry_expand_fill: atom outputs missing");
  CN_CHECK(Y_out == 0 || (row_asym && row_op && orbit_row), "cartnet_symmetry_expand_fill: row outputs missing");
  const SyLayout l = sy_layout(G, C, n_tiles);
  const char* ws = static_cast<const char*>(workspace);
  SyOut o;
  o.z = z_out; o.pos = pos_out; o.mask = non_h_mask_out; o.row_asym = row_asym; o.row_op = row_op;
  o.orbit_row = orbit_row; o.cell = cell_out;
  hipLaunchKernelGGL(cn_sy_fill, dim3((unsigned)n_tiles), dim3(SY_T), 0, ST(stream), p,
                     reinterpret_cast<const f32x4*>(ws + l.coord), reinterpret_cast<const int64_t*>(ws + l.rep),
                     reinterpret_cast<const int64_t*>(ws + l.rank_a), reinterpret_cast<const int64_t*>(ws + l.rank_h),
                     y_ptr_out, asym_site, orb_ptr, N_out, Y_out, o);
  CN_LAUNCH_CHECK("cartnet_symmetry_expand_fill");
  return 0;
}

extern "C" int cartnet_symmetry_targets(const int64_t* asym_ptr, const double* asym_ucif, const int64_t* op_ptr,
                                        const int8_t* op_rot, const double* cell, const int64_t* y_ptr,
                                        const int32_t* row_asym, const int32_t* row_op, int32_t G, int64_t Y, float* y,
                                        void* stream) {
  CN_CHECK(G >= 1 && Y >= 0, "cartnet_symmetry_targets: bad sizes (G=%d, Y=%lld)", G, (long long)Y);
  CN_CHECK(Y < (1LL << 31) * SY_T, "cartnet_symmetry_targets: too many rows for one launch");
  if (Y == 0) return 0;
  CN_CHECK(asym_ptr && asym_ucif && op_ptr && op_rot && cell && y_ptr && row_asym && row_op && y,
           "cartnet_symmetry_targets: null pointer");
  hipLaunchKernelGGL(cn_sy_targets, dim3((unsigned)((Y + SY_T - 1) / SY_T)), dim3(SY_T), 0, ST(stream), asym_ptr,
                     asym_ucif, op_ptr, op_rot, cell, y_ptr, row_asym, row_op, G, Y, y);
  CN_LAUNCH_CHECK("cartnet_symmetry_targets");
  return 0;
}

extern "C" int cartnet_symmetry_average(const float* pred, const int64_t* row_ptr, const int64_t* sel,
                                        const int64_t* site_ptr, int32_t B, int64_t M, int64_t H, const int64_t* op_ptr,
                                        const int8_t* op_rot, const int64_t* orb_ptr, const int32_t* orbit_row,
                                        const double* cell, int32_t G, int64_t S, int64_t O, float* u_cif_asym,
                                        float* spread, void* stream) {
  CN_CHECK(B >= 0 && M >= 0 && H >= 0 && G >= 1 && S >= 1 && O >= 0, "cartnet_symmetry_average: bad sizes (B=%d)", B);
  CN_CHECK(H < (1LL << 31) * SY_T, "cartnet_symmetry_average: too many sites for one launch");
  if (H == 0 || B == 0) return 0;
  CN_CHECK(pred && row_ptr && sel && site_ptr && op_ptr && op_rot && orb_ptr && orbit_row && cell && u_cif_asym && spread,
           "cartnet_symmetry_average: null pointer");
  hipLaunchKernelGGL(cn_sy_average, dim3((unsigned)((H + SY_T - 1) / SY_T)), dim3(SY_T), 0, ST(stream), pred, row_ptr,
                     sel, site_ptr, B, M, H, op_ptr, op_rot, orb_ptr, orbit_row, cell, G, S, O, u_cif_asym, spread);
  CN_LAUNCH_CHECK("cartnet_symmetry_average");
  return 0;
}

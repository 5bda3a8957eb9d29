// Periodic radius graph on the GPU (reference: dataset/utils.py:57-237 radius_graph_pbc with the cap of
// :240-360, as called by dataset/figshare_dataset.py:50-76 and by compute_knn, dataset/utils.py:456-486, one crystal at
// a time on the CPU).  ONE pass builds the graph of every crystal of (pos [N,3], cell [G,9], atom_ptr [G+1]) -- a whole
// resident shard or one batch (atom_ptr = the batch's ptr, G = its crystals) -- behind cartnet_shard_regraph_count /
// _cap / _fill; cartnet_amd/graph.py: radius_graph_csr drives it for DeviceShard.with_radius_graph, radius_graph_pbc
// and shard.pack_with_gpu_graph.
// Edges come out in the reference's order -- target atom, then source atom, then periodic image in
// cartesian_prod(a1, a2, a3) order -- so the targets are ascending and feed cartnet_csr_build directly; the ends of an
// edge are int32 atom indices inside the crystal (the shard's format), edge_ptr [G+1] the crystals' edge offsets.
// One wavefront per target atom (its crystal found by a binary search in atom_ptr), one lane per source atom (64
// sources per round); a lane walks only the periodic images that CAN lie within the radius of its pair (see "image
// box" below); the position of a lane's edges inside the row comes from a wave prefix sum of the lanes' counts, and row
// offsets are reduce-then-scan over tiles of 1024 atoms (shard_tiles.h): no atomics, identical bytes on every run.
//   count:  cn_rg_reps_kernel, cn_sr_kernel<SR_COUNT> (deg[N], *over = some row is longer than the cap), row offsets
//   cap:    cn_sr_kernel<SR_D2>, cn_cap_count_kernel (cutoff[N], deg[N] <- capped), row offsets     -- only if *over
//   fill:   cn_sr_kernel<SR_FILL>, cn_sr_edge_ptr_kernel (edge_ptr[g] = row offset of the crystal's first atom)
// The host reads the sizes between the calls.  Cutoff: a pair is kept when d^2 <= (float)(radius * radius), the product
// taken in double (cn_rg_threshold), and d^2 > 1e-4.  Cap: a row longer than max_neighbors keeps the edges with d^2 <=
// its (max_neighbors+1)-th smallest d^2 + tolerance, in their order (cn_cap_count_kernel).  A capped graph is never
// built uncapped: SR_D2 writes only the d^2 of the uncapped rows, and SR_FILL walks the images once more and emits the
// edges with d^2 <= the row's cutoff straight into the final arrays.
// Arithmetic of the distance test mirrors the reference's fp32 operation order with explicitly rounded (non-fused)
// operations; the image box only decides which candidates are tested, with a margin far above fp32 rounding.
//
// Image box.  The reference tests every image u in [-R1,R1] x [-R2,R2] x [-R3,R3] (R_d = ceil(radius |b_d|), b_d the
// reciprocal lattice vectors) against every pair: 27-125 distance tests per pair of which a handful pass.  With
// f_d = (p_i - p_j) . b_d the fractional offset of the pair, |f_d - u_d| = |(p_i - p_j - cell^T u) . b_d| <= d |b_d|, so an
// image within the radius has u_d in [f_d - radius |b_d|, f_d + radius |b_d|]: at the benchmark crystals (a ~ 13 A,
// radius 5) that is 1-2 values per axis instead of 3, ~6 tests per pair instead of 27.  Same edges, same order.
#include "common.h"
#include "shard_tiles.h"
#include <math.h>

// This file is compiled with -ffp-contract=off (cartnet_amd/build.py: EXTRA_FLAGS).  HIP's __fmul_rn / __fadd_rn are
// plain * and +, and under hipcc's default -ffp-contract=fast-honor-pragmas the compiler fused them into FMAs --
// differently in the count and the fill instantiation of a kernel, which then disagreed about a pair whose d^2 lies
// within an ulp of radius^2 (2 of 49k atoms in one 256-crystal launch: two slots of the fill pass stayed unwritten and
// every later crystal was shifted).  With contraction off every product and sum is rounded on its own, like the
// reference's torch ops, and the three instantiations of cn_sr_kernel evaluate one expression for d^2.
namespace {

constexpr int CN_RG_MAX_REPS = 16;

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }

// reps[g, d] = ceil(radius * |cross(a_{d+1}, a_{d+2}) / V|)   (dataset/utils.py:133-157)
__global__ void cn_rg_reps_kernel(const float* __restrict__ cell, int Bg, float radius, int* __restrict__ reps,
                                  float* __restrict__ recip /* [Bg][12]: b_1, b_2, b_3, radius |b_d| */) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= Bg) return;
  const float* a = cell + (size_t)g * 9;
  auto cross = [&](const float* u, const float* v, float* o) {
    o[0] = sub(mul(u[1], v[2]), mul(u[2], v[1]));
    o[1] = sub(mul(u[2], v[0]), mul(u[0], v[2]));
    o[2] = sub(mul(u[0], v[1]), mul(u[1], v[0]));
  };
  float c23[3], c31[3], c12[3];
  cross(a + 3, a + 6, c23);
  cross(a + 6, a + 0, c31);
  cross(a + 0, a + 3, c12);
  const float vol = add(add(mul(a[0], c23[0]), mul(a[1], c23[1])), mul(a[2], c23[2]));
  const float* cs[3] = {c23, c31, c12};
  for (int d = 0; d < 3; ++d) {
    const float x = cs[d][0] / vol, y = cs[d][1] / vol, z = cs[d][2] / vol;
    const float nrm = sqrtf(add(add(mul(x, x), mul(y, y)), mul(z, z)));
    // a degenerate cell (zero volume: inf / NaN here) must not become an endless image loop: repetitions are capped at
    // CN_RG_MAX_REPS (a lattice vector shorter than radius / 16 is not a crystal), NaN gives 0
    const float want = ceilf(mul(radius, nrm));
    reps[g * 3 + d] = (want >= 0.f && want <= (float)CN_RG_MAX_REPS) ? (int)want : (want > (float)CN_RG_MAX_REPS ? CN_RG_MAX_REPS : 0);
    if (recip) {
      recip[g * 12 + d * 3] = x;
      recip[g * 12 + d * 3 + 1] = y;
      recip[g * 12 + d * 3 + 2] = z;
      recip[g * 12 + 9 + d] = radius * nrm;
    }
  }
}

// One (target, source) pair: the box of periodic images that can lie within the radius and the walk over it.
struct RgPair {
  float px, py, pz, qx, qy, qz;
  int lo1, hi1, lo2, hi2, lo3, hi3;

  __device__ __forceinline__ void target(const float* __restrict__ p) { px = p[0]; py = p[1]; pz = p[2]; }

  // a lane past the last source: an empty box
  __device__ __forceinline__ void none() {
    qx = qy = qz = 0.f;
    lo1 = lo2 = lo3 = 0;
    hi1 = hi2 = hi3 = -1;
  }

  __device__ __forceinline__ void source(const float* __restrict__ q, const float* __restrict__ rb, int R1, int R2, int R3) {
    qx = q[0]; qy = q[1]; qz = q[2];
    const float ex = px - qx, ey = py - qy, ez = pz - qz;
    // fractional offset of the pair and the image interval per axis; the margin (1e-3 of a lattice step, plus 1e-5
    // relative) is four orders above the rounding of these dot products -- it only ever ADDS candidates
    const float f1 = ex * rb[0] + ey * rb[1] + ez * rb[2];
    const float f2 = ex * rb[3] + ey * rb[4] + ez * rb[5];
    const float f3 = ex * rb[6] + ey * rb[7] + ez * rb[8];
    const float m1 = rb[9] + 1e-3f + 1e-5f * fabsf(f1), m2 = rb[10] + 1e-3f + 1e-5f * fabsf(f2),
                m3 = rb[11] + 1e-3f + 1e-5f * fabsf(f3);
    // clamped in floating point before the conversion (an int conversion of inf / NaN is undefined; fmaxf / fminf
    // drop a NaN operand, which leaves the reference's full range)
    auto lo_of = [](float v, int R) { return (int)fminf((float)(R + 1), fmaxf((float)-R, ceilf(v))); };
    auto hi_of = [](float v, int R) { return (int)fmaxf((float)(-R - 1), fminf((float)R, floorf(v))); };
    lo1 = lo_of(f1 - m1, R1); hi1 = hi_of(f1 + m1, R1);
    lo2 = lo_of(f2 - m2, R2); hi2 = hi_of(f2 + m2, R2);
    lo3 = lo_of(f3 - m3, R3); hi3 = hi_of(f3 + m3, R3);
  }

  // every image of the box in cartesian_prod order (u1 slowest, u3 fastest); `emit` decides what happens to a hit
  template <class Emit>
  __device__ __forceinline__ void walk(const float* __restrict__ a, float r2, float eps2, Emit emit) const {
    for (int u1i = lo1; u1i <= hi1; ++u1i)
      for (int u2i = lo2; u2i <= hi2; ++u2i)
        for (int u3i = lo3; u3i <= hi3; ++u3i) {
          const float u1 = (float)u1i, u2 = (float)u2i, u3 = (float)u3i;
          // image offset = cell^T u, accumulated in the order of the sum, (a1 u1 + a2 u2) + a3 u3, every product and
          // sum rounded.  The reference takes it from torch.bmm (dataset/utils.py:182), whose rounding depends on the
          // BLAS code path: this order is what it gives for the 27 images of a cell wider than the radius on every host
          // measured, and for every image count on the EPYC hosts of the MI355X machines; MKL on a Xeon adds a3 u3
          // before a2 u2 from 45 images on.  The two differ by one ulp of the offset in a few per cent of the images:
          // far inside the tests' tolerance for atoms stored in their cell (|offset| <~ 2 radius), 1.3e-6 in a
          // direction for an atom stored two cells away at 0.74 A from its neighbour.
          const float ox = add(add(mul(a[0], u1), mul(a[3], u2)), mul(a[6], u3));
          const float oy = add(add(mul(a[1], u1), mul(a[4], u2)), mul(a[7], u3));
          const float oz = add(add(mul(a[2], u1), mul(a[5], u2)), mul(a[8], u3));
          const float dx = sub(px, add(qx, ox)), dy = sub(py, add(qy, oy)), dz = sub(pz, add(qz, oz));
          const float d2 = add(add(mul(dx, dx), mul(dy, dy)), mul(dz, dz));
          if ((d2 <= r2) && (d2 > eps2)) emit(dx, dy, dz, d2);
        }
  }
};

// inclusive prefix sum of the lanes' counts: lane l's edges follow those of lanes 0..l-1 (source order)
__device__ __forceinline__ int rg_lane_scan(int mine, int lane) {
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  return incl;
}

// Neighbour cap (dataset/utils.py:240-360 get_max_neighbors_mask, enforce_max_strictly = False): a target with more
// than k candidate edges keeps those with d^2 <= (k+1)-th smallest d^2 of its row + tolerance, in their original
// order; shorter rows are kept whole.  One wavefront per target.  The (k+1)-th smallest value is found by rank
// counting (every lane ranks its own elements against the whole row), which needs no sort and no scratch.
__global__ __launch_bounds__(256) void cn_cap_count_kernel(const int64_t* __restrict__ rowptr,
                                                           const float* __restrict__ d2, int N, int k, float tol,
                                                           float* __restrict__ cutoff, int* __restrict__ deg) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i >= N) return;
  const long long b = rowptr[i];
  const int n = (int)(rowptr[i + 1] - b);
  if (n <= k) {
    if (lane == 0) { cutoff[i] = INFINITY; deg[i] = n; }
    return;
  }
  const float* row = d2 + b;
  float kth = 0.f;
  bool found = false;
  for (int e = lane; e < n && !found; e += 64) {
    const float v = row[e];
    int lo = 0, eq = 0;
    for (int j = 0; j < n; ++j) {
      const float w = row[j];
      lo += (w < v);
      eq += (w == v);
    }
    if (lo <= k && k < lo + eq) { kth = v; found = true; }
  }
  // exactly the lanes holding the k-th value found it, and they all hold the same number
  const unsigned long long m = __ballot(found);
  const int owner = m ? __ffsll((long long)m) - 1 : 0;
  kth = m ? __shfl(kth, owner, 64) : INFINITY;          // m == 0 only if the row holds NaNs: keep it whole
  const float c = __fadd_rn(kth, tol);
  int cnt = 0;
  for (int e = lane; e < n; e += 64) cnt += (row[e] <= c);
  for (int off = 32; off; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if (lane == 0) { cutoff[i] = c; deg[i] = cnt; }
}

// The pass over the flat atoms of (pos, cell, atom_ptr); the protocol is at the head of the file.
enum { SR_COUNT = 0, SR_D2 = 1, SR_FILL = 2 };

__device__ __forceinline__ int64_t sr_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int MODE>
__global__ __launch_bounds__(256) void cn_sr_kernel(const float* __restrict__ pos, const float* __restrict__ cell,
                                                    const int64_t* __restrict__ atom_ptr, const int* __restrict__ reps,
                                                    const float* __restrict__ recip, int G, int N, float r2, float eps2,
                                                    int cap, int* __restrict__ deg, int64_t* __restrict__ over,
                                                    const int64_t* __restrict__ rowptr,
                                                    const float* __restrict__ cutoff, long long E,
                                                    float* __restrict__ dist_sq, int32_t* __restrict__ src,
                                                    int32_t* __restrict__ tgt, float* __restrict__ dist,
                                                    float* __restrict__ dir) {
  const int lane = threadIdx.x & 63;
  const int i1 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i1 >= N) return;
  // the crystal of the target (wave-uniform); the clamps keep a malformed atom_ptr (status 1) inside the arrays
  const int g = min(so_find(atom_ptr, 0, G + 1, (int64_t)i1), G - 1);
  const int n0 = (int)sr_clamp(atom_ptr[g], 0, i1);
  const int n = (int)sr_clamp(atom_ptr[g + 1], (int64_t)i1 + 1, N) - n0;
  const int R1 = reps[g * 3], R2 = reps[g * 3 + 1], R3 = reps[g * 3 + 2];
  const float* a = cell + (size_t)g * 9;
  const float* rb = recip + (size_t)g * 12;
  // SR_FILL keeps d^2 <= cut: +inf for an uncapped graph and for the rows the cap leaves whole
  const float cut = (MODE == SR_FILL && cutoff) ? cutoff[i1] : INFINITY;
  RgPair pr;
  pr.target(pos + (size_t)i1 * 3);
  long long out = MODE == SR_COUNT ? 0 : rowptr[i1];
  int count = 0;
  for (int base = 0; base < n; base += 64) {
    const int i2 = base + lane;
    if (i2 < n) pr.source(pos + (size_t)(n0 + i2) * 3, rb, R1, R2, R3); else pr.none();
    int mine = 0;
    pr.walk(a, r2, eps2, [&](float, float, float, float d2) { mine += d2 <= cut; });
    const int incl = rg_lane_scan(mine, lane);
    const int round_total = __shfl(incl, 63);
    if (MODE == SR_COUNT) {
      count += round_total;
      continue;
    }
    long long p = out + (incl - mine);
    pr.walk(a, r2, eps2, [&](float dx, float dy, float dz, float d2) {
      if (MODE == SR_D2) {
        if (p < E) dist_sq[p] = d2;
        ++p;
      } else if (d2 <= cut) {
        if (p < E) {
          src[p] = i2;
          tgt[p] = i1 - n0;
          const float d = sqrtf(d2);
          const float dn = fmaxf(d, 1e-12f);      // F.normalize(vec, p=2, dim=-1, eps=1e-12)
          dist[p] = d;
          dir[p * 3] = dx / dn;
          dir[p * 3 + 1] = dy / dn;
          dir[p * 3 + 2] = dz / dn;
        }
        ++p;
      }
    });
    out += round_total;
  }
  if (MODE == SR_COUNT && lane == 0) {
    deg[i1] = count;
    if (cap > 0 && count > cap) *over = 1;                   // every writer stores the same word
  }
}

// status 1: atom_ptr does not run from 0 to N in ascending steps
__global__ void cn_sr_check_kernel(const int64_t* __restrict__ atom_ptr, int G, int64_t N, int64_t* __restrict__ status) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int64_t lo = atom_ptr[g], hi = atom_ptr[g + 1];
  if (hi < lo || (g == 0 && lo != 0) || (g == G - 1 && hi != N)) *status = 1;
}

__global__ __launch_bounds__(SO_THREADS) void cn_sr_tile_sum_kernel(const int32_t* __restrict__ deg, int64_t N,
                                                                    int32_t* __restrict__ tile_sum) {
  __shared__ int lds[SO_THREADS / WAVE];
  int v[SO_ITEMS], total;
  so_load4(deg, (int64_t)blockIdx.x * SO_TILE + threadIdx.x * SO_ITEMS, N, v, 0);
  so_block_scan(v[0] + v[1] + v[2] + v[3], lds, total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(SO_THREADS) void cn_sr_tile_scan_kernel(const int32_t* __restrict__ sums, int64_t nT,
                                                                     int64_t* __restrict__ offs,
                                                                     int64_t* __restrict__ total) {
  __shared__ int64_t lds[SO_THREADS / WAVE];
  so_tile_scan(sums, nT, offs, total, lds);
}

// rowptr[i] = sum of deg[0..i) for i in [0, N] (the tile that holds item N writes the total)
__global__ __launch_bounds__(SO_THREADS) void cn_sr_rowptr_kernel(const int32_t* __restrict__ deg, int64_t N,
                                                                  const int64_t* __restrict__ tile_off,
                                                                  int64_t* __restrict__ rowptr) {
  __shared__ int lds[SO_THREADS / WAVE];
  const int64_t i0 = (int64_t)blockIdx.x * SO_TILE + threadIdx.x * SO_ITEMS;
  int v[SO_ITEMS], total;
  so_load4(deg, i0, N, v, 0);
  int64_t r = tile_off[blockIdx.x] + so_block_scan(v[0] + v[1] + v[2] + v[3], lds, total);
#pragma unroll
  for (int k = 0; k < SO_ITEMS; ++k) {
    if (i0 + k <= N) rowptr[i0 + k] = r;
    r += v[k];
  }
}

__global__ void cn_sr_edge_ptr_kernel(const int64_t* __restrict__ atom_ptr, const int64_t* __restrict__ rowptr, int G,
                                      int64_t N, int64_t* __restrict__ edge_ptr) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > G) return;
  edge_ptr[g] = rowptr[sr_clamp(atom_ptr[g], 0, N)];
}

// the workspace of a pass: [15 G] words of cn_rg_reps_kernel | deg [N] | cutoff [N] | rowptr [N+1] (uncapped) |
// rowptr_cap [N+1] | tile sums and offsets of the scans
struct SrLayout {
  int64_t nT;
  size_t reps, deg, cutoff, rowptr, rowptr_cap, tile_sum, tile_off, bytes;
};

inline size_t sr_align(size_t b) { return (b + 255) / 256 * 256; }

SrLayout sr_layout(int64_t G, int64_t N) {
  SrLayout l;
  l.nT = (N + 1 + SO_TILE - 1) / SO_TILE;                   // item domain [0, N]
  size_t o = 0;
  l.reps = o;       o += sr_align((size_t)G * 15 * 4);
  l.deg = o;        o += sr_align((size_t)(N + SO_ITEMS) * 4);
  l.cutoff = o;     o += sr_align((size_t)(N + 1) * 4);
  l.rowptr = o;     o += sr_align((size_t)(N + 1) * 8);
  l.rowptr_cap = o; o += sr_align((size_t)(N + 1) * 8);
  l.tile_sum = o;   o += sr_align((size_t)(l.nT + SO_ITEMS) * 4);
  l.tile_off = o;   o += sr_align((size_t)(l.nT + 1) * 8);
  l.bytes = o;
  return l;
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

// The reference keeps a pair when d^2 <= radius * radius with the product taken in double (a Python float,
// dataset/utils.py:202) and rounded to fp32 once, for the comparison with the fp32 d^2.  The fp32 product of the rounded
// radius is one ulp larger for some radii (3.7: 13.6899996 against 13.6900005), so the radius crosses the ABI in double;
// the repetition counts use the fp32 product radius |b_d|, as the reference's tensor arithmetic does (:140).
static float cn_rg_threshold(double radius) { return (float)(radius * radius); }

static int sr_check(const float* pos, const float* cell, const int64_t* atom_ptr, int32_t G, int64_t N, double radius,
                    const void* ws, size_t ws_bytes, const char* who) {
  CN_CHECK(G >= 1 && N >= 0 && N < (1LL << 31) - SO_TILE && radius > 0.0, "%s: bad sizes (G=%d)", who, G);
  CN_CHECK(cell && atom_ptr && (N == 0 || pos), "%s: the shard needs pos, cell and atom_ptr", who);
  CN_CHECK(ws && ws_bytes >= sr_layout(G, N).bytes, "%s: workspace too small", who);
  CN_CHECK(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "%s: workspace must be 16-byte aligned", who);
  return 0;
}

// rowptr[0..N] = exclusive prefix sum of deg, *total = rowptr[N]
static int sr_row_offsets(const SrLayout& l, char* ws, int64_t N, int64_t* rowptr, int64_t* total, hipStream_t st,
                          const char* who) {
  const int32_t* deg = reinterpret_cast<const int32_t*>(ws + l.deg);
  int32_t* tile_sum = reinterpret_cast<int32_t*>(ws + l.tile_sum);
  int64_t* tile_off = reinterpret_cast<int64_t*>(ws + l.tile_off);
  hipLaunchKernelGGL(cn_sr_tile_sum_kernel, dim3((unsigned)l.nT), dim3(SO_THREADS), 0, st, deg, N, tile_sum);
  CN_LAUNCH_CHECK(who);
  hipLaunchKernelGGL(cn_sr_tile_scan_kernel, dim3(1), dim3(SO_THREADS), 0, st, tile_sum, l.nT, tile_off, total);
  CN_LAUNCH_CHECK(who);
  hipLaunchKernelGGL(cn_sr_rowptr_kernel, dim3((unsigned)l.nT), dim3(SO_THREADS), 0, st, deg, N, tile_off, rowptr);
  CN_LAUNCH_CHECK(who);
  return 0;
}

extern "C" size_t cartnet_shard_regraph_workspace_bytes(int32_t G, int64_t N, int64_t E_uncapped) {
  if (G < 1 || N < 0 || E_uncapped < 0) return 0;
  return sr_layout(G, N).bytes + sr_align((size_t)E_uncapped * 4);
}

extern "C" int cartnet_shard_regraph_count(const float* pos, const float* cell, const int64_t* atom_ptr, int32_t G,
                                           int64_t N, double radius, int32_t max_neighbors, void* workspace,
                                           size_t workspace_bytes, int64_t* totals, void* stream) {
  if (sr_check(pos, cell, atom_ptr, G, N, radius, workspace, workspace_bytes, "cartnet_shard_regraph_count")) return 1;
  CN_CHECK(totals, "cartnet_shard_regraph_count: null totals");
  const SrLayout l = sr_layout(G, N);
  char* ws = static_cast<char*>(workspace);
  int* reps = reinterpret_cast<int*>(ws + l.reps);
  float* recip = reinterpret_cast<float*>(reps + 3 * (size_t)G);
  if (hipMemsetAsync(totals, 0, 4 * sizeof(int64_t), ST(stream)) != hipSuccess) {
    cartnet_set_error("cartnet_shard_regraph_count: hipMemsetAsync failed");
    return 2;
  }
  hipLaunchKernelGGL(cn_sr_check_kernel, dim3(cn_ceil_div(G, 256)), dim3(256), 0, ST(stream), atom_ptr, (int)G, N, totals + 3);
  CN_LAUNCH_CHECK("cartnet_shard_regraph_count/check");
  hipLaunchKernelGGL(cn_rg_reps_kernel, dim3(cn_ceil_div(G, 64)), dim3(64), 0, ST(stream), cell, (int)G, (float)radius, reps, recip);
  CN_LAUNCH_CHECK("cartnet_shard_regraph_count/reps");
  if (N > 0) {
    hipLaunchKernelGGL(cn_sr_kernel<SR_COUNT>, dim3(cn_ceil_div(N, 4)), dim3(256), 0, ST(stream), pos, cell, atom_ptr, reps,
                       recip, (int)G, (int)N, cn_rg_threshold(radius), 0.0001f, (int)max_neighbors,
                       reinterpret_cast<int*>(ws + l.deg), totals + 2, (const int64_t*)nullptr, (const float*)nullptr, 0LL,
                       (float*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr, (float*)nullptr);
    CN_LAUNCH_CHECK("cartnet_shard_regraph_count/degrees");
  }
  return sr_row_offsets(l, ws, N, reinterpret_cast<int64_t*>(ws + l.rowptr), totals, ST(stream),
                        "cartnet_shard_regraph_count/offsets");
}

extern "C" int cartnet_shard_regraph_cap(const float* pos, const float* cell, const int64_t* atom_ptr, int32_t G,
                                         int64_t N, double radius, int32_t max_neighbors, float tolerance,
                                         int64_t E_uncapped, void* workspace, size_t workspace_bytes, float* dist_sq,
                                         int64_t* totals, void* stream) {
  if (sr_check(pos, cell, atom_ptr, G, N, radius, workspace, workspace_bytes, "cartnet_shard_regraph_cap")) return 1;
  CN_CHECK(max_neighbors >= 1 && tolerance >= 0.f && E_uncapped >= 0 && totals, "cartnet_shard_regraph_cap: bad arguments");
  CN_CHECK(E_uncapped == 0 || dist_sq, "cartnet_shard_regraph_cap: null dist_sq");
  const SrLayout l = sr_layout(G, N);
  char* ws = static_cast<char*>(workspace);
  const int* reps = reinterpret_cast<const int*>(ws + l.reps);
  const float* recip = reinterpret_cast<const float*>(reps + 3 * (size_t)G);
  const int64_t* rowptr = reinterpret_cast<const int64_t*>(ws + l.rowptr);
  if (N > 0) {
    hipLaunchKernelGGL(cn_sr_kernel<SR_D2>, dim3(cn_ceil_div(N, 4)), dim3(256), 0, ST(stream), pos, cell, atom_ptr, reps,
                       recip, (int)G, (int)N, cn_rg_threshold(radius), 0.0001f, 0, (int*)nullptr, (int64_t*)nullptr, rowptr,
                       (const float*)nullptr, (long long)E_uncapped, dist_sq, (int32_t*)nullptr, (int32_t*)nullptr,
                       (float*)nullptr, (float*)nullptr);
    CN_LAUNCH_CHECK("cartnet_shard_regraph_cap/dist_sq");
    hipLaunchKernelGGL(cn_cap_count_kernel, dim3(cn_ceil_div(N, 4)), dim3(256), 0, ST(stream), rowptr, dist_sq, (int)N,
                       (int)max_neighbors, tolerance, reinterpret_cast<float*>(ws + l.cutoff),
                       reinterpret_cast<int*>(ws + l.deg));
    CN_LAUNCH_CHECK("cartnet_shard_regraph_cap/cutoff");
  }
  return sr_row_offsets(l, ws, N, reinterpret_cast<int64_t*>(ws + l.rowptr_cap), totals + 1, ST(stream),
                        "cartnet_shard_regraph_cap/offsets");
}

extern "C" int cartnet_shard_regraph_fill(const float* pos, const float* cell, const int64_t* atom_ptr, int32_t G,
                                          int64_t N, double radius, int32_t capped, const void* workspace,
                                          size_t workspace_bytes, int64_t E, int64_t* edge_ptr, int32_t* edge_src,
                                          int32_t* edge_tgt, float* cart_dist, float* cart_dir, void* stream) {
  if (sr_check(pos, cell, atom_ptr, G, N, radius, workspace, workspace_bytes, "cartnet_shard_regraph_fill")) return 1;
  CN_CHECK(E >= 0 && edge_ptr, "cartnet_shard_regraph_fill: bad arguments");
  CN_CHECK(E == 0 || (edge_src && edge_tgt && cart_dist && cart_dir), "cartnet_shard_regraph_fill: edge outputs missing");
  const SrLayout l = sr_layout(G, N);
  const char* ws = static_cast<const char*>(workspace);
  const int* reps = reinterpret_cast<const int*>(ws + l.reps);
  const float* recip = reinterpret_cast<const float*>(reps + 3 * (size_t)G);
  const int64_t* rowptr = reinterpret_cast<const int64_t*>(ws + (capped ? l.rowptr_cap : l.rowptr));
  const float* cutoff = capped ? reinterpret_cast<const float*>(ws + l.cutoff) : nullptr;
  if (N > 0 && E > 0) {
    hipLaunchKernelGGL(cn_sr_kernel<SR_FILL>, dim3(cn_ceil_div(N, 4)), dim3(256), 0, ST(stream), pos, cell, atom_ptr, reps,
                       recip, (int)G, (int)N, cn_rg_threshold(radius), 0.0001f, 0, (int*)nullptr, (int64_t*)nullptr, rowptr,
                       cutoff, (long long)E, (float*)nullptr, edge_src, edge_tgt, cart_dist, cart_dir);
    CN_LAUNCH_CHECK("cartnet_shard_regraph_fill/edges");
  }
  hipLaunchKernelGGL(cn_sr_edge_ptr_kernel, dim3(cn_ceil_div((int64_t)G + 1, 256)), dim3(256), 0, ST(stream), atom_ptr, rowptr,
                     (int)G, N, edge_ptr);
  CN_LAUNCH_CHECK("cartnet_shard_regraph_fill/edge_ptr");
  return 0;
}

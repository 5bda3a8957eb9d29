// Whole-shard transforms on the resident dataset (cartnet_amd/shard.py): every crystal in the frame of its canonical
// reduced lattice -- the iComformer dataset recipe.
//
// Reference: dataset/datasetADP.py:75-80 (DatasetADP.get with optimize_cell=True) calls optmize_lattice
// (dataset/utils.py:366-452) for ONE crystal per access on the host: 124 stacked candidate vectors, an argsort, two Python
// loops over them with a handful of tiny tensor ops each, then cart_dir @ R and R^T y R.  Here:
//
//   select:  cn_lo_select   one wavefront per crystal.  A lane holds two of the 124 candidates i c0 + j c1 + k c2
//                           (i, j, k in -2..2, k fastest, (0,0,0) skipped); a candidate's rank is the number of candidates
//                           with a smaller (norm, enumeration index), counted against the other lanes' values -- no sort.
//                           "First admissible candidate in rank order" is a wave-wide minimum of the rank over the lanes
//                           whose predicate holds; three rounds give v1, v2, v3.  Then the sign and handedness rules and
//                           the frame (rows x = v1/|v1|, y = normalised part of v2 orthogonal to x, z = x cross y).
//                           Writes cell' = [v1;v2;v3] R^T, R, the signed integer coefficients of the three vectors and a
//                           status per crystal (1 = no admissible second or third vector).
//            cn_lo_status   one workgroup: the first crystal with a non-zero status, or -1, as ONE word for the host.
//   rotate:  cn_lo_rotate   the hot path: cart_dir[e] <- cart_dir[e] R[g(e)] over all edges and y[m] <- R^T y[m] R over all
//                           target rows, one launch each.  Tiles of 1024 items, 256 threads x 4 consecutive items, so a thread's
//                           48 (144) bytes are three (nine) 16-byte loads and stores; the crystal of an item comes from the
//                           binary search of shard_tiles.h in edge_ptr / y_ptr; int64 offsets.  HBM-bound: 12 B in + 12 B
//                           out per edge, 36 B + 36 B per target row; R (36 B per crystal) stays in cache.
//
// No atomics, no workgroup waits for another, every output is a pure function of the input: two runs give the same bytes.
//
// This file is compiled with -ffp-contract=off (build.py): the candidates ((i c0) + (j c1)) + (k c2) and their norms
// sqrt((x x + y y) + z z) are then the host rule's fp32 values bit for bit (cartnet_amd/data.py: lattice_basis), so the
// GPU orders the candidates as the host does wherever two norms are not within rounding of each other.  The rotation
// products are the unfused sums torch computes as well.
#include "common.h"
#include "shard_tiles.h"

namespace {

constexpr int LO_CAND = 124;
constexpr int LO_NONE = 255;                  // larger than every rank
constexpr float LO_ATOL = 1e-3f;              // torch.isclose(..., 0, atol=1e-3), dataset/utils.py:432,441
constexpr float LO_HALF_PI = 1.57079637f;     // the reference compares an fp32 angle with pi / 2 in fp32

struct LoVec {
  float x, y, z;
  int e;                                      // enumeration index 0..123
};

__device__ __forceinline__ void lo_coeffs(int e, int& i, int& j, int& k) {
  const int f = e + (e >= 62);                // (0,0,0) is position 62 of the full 5 x 5 x 5 nest
  i = f / 25 - 2;
  j = (f / 5) % 5 - 2;
  k = f % 5 - 2;
}

__device__ __forceinline__ float lo_dot(float ax, float ay, float az, float bx, float by, float bz) {
  return (ax * bx + ay * by) + az * bz;
}

__device__ __forceinline__ void lo_cross(float ax, float ay, float az, float bx, float by, float bz, float& cx, float& cy,
                                         float& cz) {
  cx = ay * bz - az * by;
  cy = az * bx - ax * bz;
  cz = ax * by - ay * bx;
}

__device__ __forceinline__ float lo_norm(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

__device__ __forceinline__ int lo_wave_min(int v) {
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1) {
    const int t = __shfl_xor(v, d, WAVE);
    v = t < v ? t : v;
  }
  return v;
}

// vector_angle(v1, w) > pi / 2 (dataset/utils.py:410-412,433-437): w is negated
__device__ __forceinline__ bool lo_flips(const LoVec& v1, float n1, const LoVec& w) {
  const float c = lo_dot(v1.x, v1.y, v1.z, w.x, w.y, w.z) / (n1 * lo_norm(w.x, w.y, w.z));
  return fabsf(acosf(c)) > LO_HALF_PI;
}

__global__ __launch_bounds__(256) void cn_lo_select(const float* __restrict__ cell, int G, float* __restrict__ cell_out,
                                                    float* __restrict__ rot_out, int8_t* __restrict__ basis_out,
                                                    int32_t* __restrict__ status) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int g = blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6);
  if (g >= G) return;                                          // wave-uniform; the kernel has no workgroup barrier
  float c[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) c[q] = cell[(size_t)g * 9 + q];
  // this lane's two candidates: e = lane and lane + 64 (the last four lanes hold one)
  float vx[2], vy[2], vz[2], nn[2];
  int rank[2] = {0, 0};
  bool valid[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int e = lane + WAVE * p;
    valid[p] = e < LO_CAND;
    int i, j, k;
    lo_coeffs(valid[p] ? e : 0, i, j, k);
    const float fi = (float)i, fj = (float)j, fk = (float)k;
    vx[p] = (fi * c[0] + fj * c[3]) + fk * c[6];
    vy[p] = (fi * c[1] + fj * c[4]) + fk * c[7];
    vz[p] = (fi * c[2] + fj * c[5]) + fk * c[8];
    nn[p] = valid[p] ? lo_norm(vx[p], vy[p], vz[p]) : __builtin_inff();
  }
  // rank = number of candidates that come first in the (norm, enumeration index) order; a total order even with NaNs
  for (int s = 0; s < WAVE; ++s) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const float on = __shfl(nn[p], s, WAVE);
      const int oe = s + WAVE * p;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int e = lane + WAVE * q;
        rank[q] += (on < nn[q]) || (!(nn[q] < on) && oe < e);
      }
    }
  }
  // the candidate of rank r, in every lane
  auto pick = [&](int r) {
    const bool m1 = rank[1] == r;
    const int owner = __ffsll((unsigned long long)__ballot(rank[0] == r || m1)) - 1;       // ranks are a permutation
    LoVec v;
    v.x = __shfl(m1 ? vx[1] : vx[0], owner, WAVE);
    v.y = __shfl(m1 ? vy[1] : vy[0], owner, WAVE);
    v.z = __shfl(m1 ? vz[1] : vz[0], owner, WAVE);
    v.e = __shfl(m1 ? lane + WAVE : lane, owner, WAVE);
    return v;
  };
  const LoVec v1 = pick(0);                                               // closest_vectors[0]
  const float n1 = lo_norm(v1.x, v1.y, v1.z);
  // v2: the next candidate that is not collinear with v1
  int key = LO_NONE;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    float cx, cy, cz;
    lo_cross(v1.x, v1.y, v1.z, vx[p], vy[p], vz[p], cx, cy, cz);
    const bool ok = valid[p] && rank[p] > 0 && !(lo_norm(cx, cy, cz) <= LO_ATOL);
    key = ok && rank[p] < key ? rank[p] : key;
  }
  const int r2 = lo_wave_min(key);
  int r3 = LO_NONE;
  LoVec v2 = v1, v3 = v1;
  float s2 = 1.f, s3 = 1.f;
  float nx = 0.f, ny = 0.f, nz = 0.f;
  if (r2 != LO_NONE) {
    v2 = pick(r2);
    s2 = lo_flips(v1, n1, v2) ? -1.f : 1.f;
    v2.x *= s2; v2.y *= s2; v2.z *= s2;
    lo_cross(v1.x, v1.y, v1.z, v2.x, v2.y, v2.z, nx, ny, nz);
    // v3: the next candidate outside the plane of v1 and v2.  The reference restarts one element before v2
    // (closest_vectors[i:]); that element and v2 itself lie in the plane and are rejected again, so the search in effect
    // starts after v2.
    key = LO_NONE;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const bool ok = valid[p] && rank[p] > r2 && !(fabsf(lo_dot(nx, ny, nz, vx[p], vy[p], vz[p])) <= LO_ATOL);
      key = ok && rank[p] < key ? rank[p] : key;
    }
    r3 = lo_wave_min(key);
  }
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, L[9];
  int B[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 9; ++q) L[q] = c[q];                                // a degenerate cell is passed through
  const bool ok = r3 != LO_NONE;
  if (ok) {
    v3 = pick(r3);
    s3 = lo_flips(v1, n1, v3) ? -1.f : 1.f;
    v3.x *= s3; v3.y *= s3; v3.z *= s3;
    // find_right_hand_system (dataset/utils.py:414-418)
    const float h = lo_dot(nx, ny, nz, v3.x, v3.y, v3.z) < 0.f ? -1.f : 1.f;
    const float V[9] = {h * v1.x, h * v1.y, h * v1.z, h * v2.x, h * v2.y, h * v2.z, h * v3.x, h * v3.y, h * v3.z};
    const int sg[3] = {(int)h, (int)(h * s2), (int)(h * s3)};
    const int en[3] = {v1.e, v2.e, v3.e};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      int i, j, k;
      lo_coeffs(en[r], i, j, k);
      B[r * 3] = sg[r] * i; B[r * 3 + 1] = sg[r] * j; B[r * 3 + 2] = sg[r] * k;
    }
    // rotate_crystal_to_lattice (dataset/utils.py:366-398)
    const float na = lo_norm(V[0], V[1], V[2]);
    R[0] = V[0] / na; R[1] = V[1] / na; R[2] = V[2] / na;
    const float d = lo_dot(V[3], V[4], V[5], R[0], R[1], R[2]);
    const float px = V[3] - d * R[0], py = V[4] - d * R[1], pz = V[5] - d * R[2];
    const float np = lo_norm(px, py, pz);
    R[3] = px / np; R[4] = py / np; R[5] = pz / np;
    lo_cross(R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8]);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q)                                         // [v1;v2;v3] R^T
        L[r * 3 + q] = lo_dot(V[r * 3], V[r * 3 + 1], V[r * 3 + 2], R[q * 3], R[q * 3 + 1], R[q * 3 + 2]);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      cell_out[(size_t)g * 9 + q] = L[q];
      rot_out[(size_t)g * 9 + q] = R[q];
      basis_out[(size_t)g * 9 + q] = (int8_t)B[q];
    }
    status[g] = ok ? 0 : 1;
  }
}

// *first_bad = the first crystal whose status is not 0, or -1; one workgroup
__global__ __launch_bounds__(SO_THREADS) void cn_lo_status(const int32_t* __restrict__ status, int G,
                                                           int64_t* __restrict__ first_bad) {
  __shared__ int lds[SO_THREADS / WAVE];
  int first = INT32_MAX;
  for (int g = threadIdx.x; g < G; g += SO_THREADS)
    if (status[g] != 0 && g < first) first = g;
  first = lo_wave_min(first);
  if ((threadIdx.x & (WAVE - 1)) == 0) lds[threadIdx.x >> 6] = first;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < SO_THREADS / WAVE; ++w) first = lds[w] < first ? lds[w] : first;
    *first_bad = first == INT32_MAX ? -1 : first;
  }
}

// v' = v R  (row vector times 3x3), as collate.hip's rot_row
__device__ __forceinline__ void lo_rot_row(const float* v, const float* R, float* o) {
#pragma unroll
  for (int j = 0; j < 3; ++j) o[j] = v[0] * R[j] + v[1] * R[3 + j] + v[2] * R[6 + j];
}

// W floats per item (3: a direction, 9: a 3x3 target); a thread owns SO_ITEMS consecutive items = W 16-byte vectors
template <int W>
__device__ __forceinline__ void lo_rotate_items(const float* __restrict__ in, float* __restrict__ out,
                                                const int64_t* __restrict__ ptr, int G, int64_t n,
                                                const float* __restrict__ rot, int64_t t0) {
  const int64_t i0 = t0 + threadIdx.x * SO_ITEMS;
  if (i0 >= n) return;
  const bool full = i0 + SO_ITEMS <= n;
  float v[W * SO_ITEMS], o[W * SO_ITEMS];
  if (full) {
#pragma unroll
    for (int q = 0; q < W; ++q) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(in + i0 * W + q * 4);
      v[q * 4] = t.x; v[q * 4 + 1] = t.y; v[q * 4 + 2] = t.z; v[q * 4 + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < W * SO_ITEMS; ++q) v[q] = i0 * W + q < n * W ? in[i0 * W + q] : 0.f;
  }
  int g = so_first_crystal(ptr, G, n, t0, i0);                  // i0 < n: g < G
  int loaded = -1;
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
#pragma unroll
  for (int k = 0; k < SO_ITEMS; ++k) {
    const int64_t i = i0 + k;
    if (i < n) {
      while (g < G - 1 && ptr[g + 1] <= i) ++g;
      if (g != loaded) {
#pragma unroll
        for (int q = 0; q < 9; ++q) R[q] = rot[(size_t)g * 9 + q];
        loaded = g;
      }
    }
    const float* a = v + k * W;
    float* b = o + k * W;
    if (W == 3) {
      lo_rot_row(a, R, b);
    } else {                                                     // R^T (y R), as cartnet_collate's augmentation
      float t[9];
#pragma unroll
      for (int r = 0; r < 3; ++r) lo_rot_row(a + 3 * r, R, t + 3 * r);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) b[r * 3 + q] = R[r] * t[q] + R[3 + r] * t[3 + q] + R[6 + r] * t[6 + q];
    }
  }
  if (full) {
#pragma unroll
    for (int q = 0; q < W; ++q) {
      f32x4 t;
      t.x = o[q * 4]; t.y = o[q * 4 + 1]; t.z = o[q * 4 + 2]; t.w = o[q * 4 + 3];
      *reinterpret_cast<f32x4*>(out + i0 * W + q * 4) = t;
    }
  } else {
#pragma unroll
    for (int q = 0; q < W * SO_ITEMS; ++q)
      if (i0 * W + q < n * W) out[i0 * W + q] = o[q];
  }
}

// one instantiation per item width: the 3x3 targets need three times the registers of the directions, and the edges,
// which are nearly all of the traffic, should not run at that occupancy
template <int W>
__global__ __launch_bounds__(SO_THREADS) void cn_lo_rotate(const float* __restrict__ in, float* __restrict__ out,
                                                           const int64_t* __restrict__ ptr, int G, int64_t n,
                                                           const float* __restrict__ rot) {
  lo_rotate_items<W>(in, out, ptr, G, n, rot, (int64_t)blockIdx.x * SO_TILE);
}

#define ST(s) reinterpret_cast<hipStream_t>(s)

inline bool lo_aligned(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" int cartnet_shard_optimize_cell_select(const float* cell, int32_t G, float* cell_out, float* rotation,
                                                  int8_t* basis, int32_t* status, int64_t* first_bad, void* stream) {
  CN_CHECK(G >= 1, "cartnet_shard_optimize_cell_select: bad sizes (G=%d)", G);
  CN_CHECK(cell && cell_out && rotation && basis && status && first_bad,
           "cartnet_shard_optimize_cell_select: null argument");
  hipLaunchKernelGGL(cn_lo_select, dim3((unsigned)cn_ceil_div(G, 256 / WAVE)), dim3(256), 0, ST(stream), cell, G, cell_out,
                     rotation, basis, status);
  CN_LAUNCH_CHECK("cartnet_shard_optimize_cell_select/select");
  hipLaunchKernelGGL(cn_lo_status, dim3(1), dim3(SO_THREADS), 0, ST(stream), status, G, first_bad);
  CN_LAUNCH_CHECK("cartnet_shard_optimize_cell_select/status");
  return 0;
}

extern "C" int cartnet_shard_optimize_cell_rotate(const CartnetShard* shard, int32_t G, int64_t E, int64_t M,
                                                  const float* rotation, float* cart_dir_out, float* y_out,
                                                  void* stream) {
  CN_CHECK(shard && rotation, "cartnet_shard_optimize_cell_rotate: null argument");
  CN_CHECK(G >= 1 && E >= 0 && M >= 0, "cartnet_shard_optimize_cell_rotate: bad sizes (G=%d)", G);
  CN_CHECK(E < (1LL << 40) && M < (1LL << 40), "cartnet_shard_optimize_cell_rotate: shard too large for one launch");
  CN_CHECK(shard->edge_ptr && (E == 0 || (shard->cart_dir && cart_dir_out)),
           "cartnet_shard_optimize_cell_rotate: edge arrays missing");
  const bool targets = y_out != nullptr && M > 0;
  CN_CHECK(!y_out || (shard->y_width == 9 && shard->y_ptr && (M == 0 || shard->y)),
           "cartnet_shard_optimize_cell_rotate: y_out needs per-atom 3x3 targets (y_width 9)");
  CN_CHECK(lo_aligned(shard->cart_dir) && lo_aligned(cart_dir_out) && lo_aligned(shard->y) && lo_aligned(y_out),
           "cartnet_shard_optimize_cell_rotate: arrays must be 16-byte aligned");
  if (E > 0) {
    hipLaunchKernelGGL(cn_lo_rotate<3>, dim3((unsigned)((E + SO_TILE - 1) / SO_TILE)), dim3(SO_THREADS), 0, ST(stream),
                       shard->cart_dir, cart_dir_out, shard->edge_ptr, G, E, rotation);
    CN_LAUNCH_CHECK("cartnet_shard_optimize_cell_rotate/edges");
  }
  if (targets) {
    hipLaunchKernelGGL(cn_lo_rotate<9>, dim3((unsigned)((M + SO_TILE - 1) / SO_TILE)), dim3(SO_THREADS), 0, ST(stream),
                       shard->y, y_out, shard->y_ptr, G, M, rotation);
    CN_LAUNCH_CHECK("cartnet_shard_optimize_cell_rotate/targets");
  }
  return 0;
}

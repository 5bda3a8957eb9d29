// The tiling that the whole-shard passes share (shard_ops.hip, lattice_ops.hip): a workgroup of 256 threads owns a tile
// of 1024 consecutive items (atoms, edges, target rows), a thread 4 consecutive ones, and an item finds its crystal by a
// binary search in the [G+1] int64 offsets narrowed to the crystals its tile touches.  The prefix sums of these passes
// (and of the shard-wide radius graph, radius_graph.hip) are reduce-then-scan over such tiles: tile sums, one scan of the
// sums by a single workgroup (so_tile_scan), a pass that adds the tile's carry.
#pragma once
#include "common.h"

constexpr int SO_THREADS = 256;
constexpr int SO_ITEMS = 4;
constexpr int SO_TILE = SO_THREADS * SO_ITEMS;

// largest g in [lo, hi) with ptr[g] <= i; requires ptr[lo] <= i and (hi == G + 1 or i < ptr[hi])
__device__ __forceinline__ int so_find(const int64_t* __restrict__ ptr, int lo, int hi, int64_t i) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// crystal of item i0 = the first item of this thread, searched among the crystals the tile [t0, t0 + 1024) touches
__device__ __forceinline__ int so_first_crystal(const int64_t* __restrict__ ptr, int G, int64_t n, int64_t t0, int64_t i0) {
  const int64_t t1 = t0 + SO_TILE - 1 < n ? t0 + SO_TILE - 1 : n;
  const int g_lo = so_find(ptr, 0, G + 1, t0);
  const int g_hi = so_find(ptr, g_lo, G + 1, t1);
  return so_find(ptr, g_lo, g_hi + 1, i0);
}

// The crystal walk of a row kernel whose thread takes its items in ascending order: so_walk_first gives the crystal of the
// thread's first item i0 (never beyond the last crystal), so_walk_to steps from the crystal g of an earlier item to the
// crystal of item i, over empty crystals.
__device__ __forceinline__ int so_walk_first(const int64_t* __restrict__ ptr, int G, int64_t n, int64_t t0, int64_t i0) {
  const int g = so_first_crystal(ptr, G, n, t0, i0);
  return g > G - 1 ? G - 1 : g;
}

__device__ __forceinline__ int so_walk_to(const int64_t* __restrict__ ptr, int G, int g, int64_t i) {
  while (g < G - 1 && ptr[g + 1] <= i) ++g;
  return g;
}

typedef int i32x4 __attribute__((ext_vector_type(4)));

// inclusive scan over the 64 lanes of a wavefront
template <class T>
__device__ __forceinline__ T so_wave_scan(T v, int lane) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const T t = __shfl_up(v, d, WAVE);
    if (lane >= d) v += t;
  }
  return v;
}

// exclusive prefix of v over the workgroup's 256 threads, `total` = the workgroup's sum; lds: 4 words, reusable on return
template <class T>
__device__ __forceinline__ T so_block_scan(T v, T* lds, T& total) {
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x >> 6;
  const T inc = so_wave_scan(v, lane);
  if (lane == WAVE - 1) lds[wid] = inc;
  __syncthreads();
  T off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < SO_THREADS / WAVE; ++w) {
    const T s = lds[w];
    if (w < wid) off += s;
    tot += s;
  }
  __syncthreads();
  total = tot;
  return off + inc - v;
}

__device__ __forceinline__ void so_load4(const int32_t* __restrict__ a, int64_t i0, int64_t n, int v[SO_ITEMS], int fill) {
  if (i0 + SO_ITEMS <= n) {
    const i32x4 t = *reinterpret_cast<const i32x4*>(a + i0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < SO_ITEMS; ++k) v[k] = i0 + k < n ? a[i0 + k] : fill;
  }
}

// offs[t] = sum of sums[0..t), offs[nT] = *total = the sum of all; the body of a one-workgroup kernel (lds: 4 words).
// The sums of a round are added in int64: a tile of 1024 atom degrees (radius_graph.hip) can be far above 1024
__device__ __forceinline__ void so_tile_scan(const int32_t* __restrict__ sums, int64_t nT, int64_t* __restrict__ offs,
                                             int64_t* __restrict__ total, int64_t* lds) {
  int64_t carry = 0;
  for (int64_t base = 0; base < nT; base += SO_TILE) {
    const int64_t i0 = base + threadIdx.x * SO_ITEMS;
    int v[SO_ITEMS];
    so_load4(sums, i0, nT, v, 0);
    int64_t tot;
    int64_t r = carry + so_block_scan((int64_t)v[0] + v[1] + v[2] + v[3], lds, tot);
#pragma unroll
    for (int k = 0; k < SO_ITEMS; ++k) {
      if (i0 + k < nT) offs[i0 + k] = r;
      r += v[k];
    }
    carry += tot;
  }
  if (threadIdx.x == 0) {
    offs[nT] = carry;
    *total = carry;
  }
}

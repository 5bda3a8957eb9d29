// The tiling that the whole-shard passes share (shard_ops.hip, lattice_ops.hip): a workgroup of 256 threads owns a tile
// of 1024 consecutive items (atoms, edges, target rows), a thread 4 consecutive ones, and an item finds its crystal by a
// binary search in the [G+1] int64 offsets narrowed to the crystals its tile touches.
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

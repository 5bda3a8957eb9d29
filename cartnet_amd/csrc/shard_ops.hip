// Whole-shard transforms on the resident dataset (cartnet_amd/shard.py): the hydrogen-free copy of a shard.
//
// Reference: dataset/datasetADP.py:49-72 (DatasetADP.get with hydrogens=False) removes the hydrogens of ONE crystal
// per access on the host -- a boolean mask over the atoms, torch.isin over the edges, a Python dict and a list
// comprehension that renumbers every surviving edge.  Here the same rule is a stable compaction of the whole shard:
//
//   count:  cn_so_atom_count   per tile of 1024 atoms, the number kept (z != 1); checks a stored non_h_mask against it
//           cn_so_tile_scan    exclusive scan of the tile sums (one workgroup, int64 carry)
//           cn_so_atom_rank    wavefront / LDS scan inside the tile + the tile's carry -> rank[a] (int64, -1 = dropped)
//                              and atom_ptr' (the rank at every crystal's first atom)
//           cn_so_edge_count   per tile of 1024 edges, the number whose two ends are kept
//           cn_so_tile_scan    the same scan over the edge tiles; the two totals land next to the status word
//   fill:   cn_so_atom_fill    z, pos, mask of the kept atoms to rank[a]
//           cn_so_edge_fill    flags again, scan inside the tile + carry, scatter of the kept edges (renumbered to
//                              rank[end] - atom_ptr'[crystal]) and edge_ptr'
//
// Reduce-then-scan: no workgroup ever waits for another one, there is no atomic, and every output position is a pure
// function of the input, so two runs give the same bytes.  A thread owns 4 CONSECUTIVE items, which keeps the order
// (the compaction is stable: edge_tgt stays ascending per crystal) and makes its loads 16-byte vectors (z, edge_src,
// edge_tgt, cart_dist: one each; cart_dir / pos: its 4 rows are 3 of them).  An item finds its crystal by a binary search
// in the offsets narrowed to the crystals its tile touches, then walks forward.  Item domains are [0, N] and [0, E]
// INCLUSIVE: the one-past-the-end item is never kept, its exclusive rank is the total, and the thread that owns it
// writes the offsets of the crystals that start there (empty ones at the end of the shard, and entry G).
// Memory-bound: 8 B read per edge in count (+ two cached 8-byte rank gathers), 24 B read + 24 B per kept edge in fill.
#include "common.h"
#include "shard_tiles.h"

namespace {

__device__ __forceinline__ void so_block_sum_store(int v, int* lds, int32_t* out) {
  int total;
  so_block_scan(v, lds, total);
  if (threadIdx.x == 0) *out = total;
}

// the offsets of the crystals that start at item i (crystal g and the empty ones right before it) are `rank`
__device__ __forceinline__ void so_store_starts(const int64_t* __restrict__ ptr, int64_t* __restrict__ out, int g,
                                                int64_t i, int64_t rank) {
  for (int q = g; q >= 0 && ptr[q] == i; --q) out[q] = rank;
}

// ---------------------------------------------------------------------------------------------------- atoms
__global__ __launch_bounds__(SO_THREADS) void cn_so_atom_count(const int32_t* __restrict__ z,
                                                               const uint8_t* __restrict__ mask, int64_t N,
                                                               int32_t* __restrict__ tile_sum,
                                                               int64_t* __restrict__ status) {
  __shared__ int lds[SO_THREADS / WAVE];
  const int64_t i0 = (int64_t)blockIdx.x * SO_TILE + threadIdx.x * SO_ITEMS;
  int zz[SO_ITEMS];
  so_load4(z, i0, N, zz, 1);                                 // past the end: counted as dropped
  int cnt = 0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < SO_ITEMS; ++k) {
    const bool keep = zz[k] != 1;
    cnt += keep;
    if (mask && i0 + k < N) bad |= (mask[i0 + k] != 0) != keep;
  }
  if (bad) *status = 1;                                      // every writer stores the same word
  so_block_sum_store(cnt, lds, tile_sum + blockIdx.x);
}

__global__ __launch_bounds__(SO_THREADS) void cn_so_tile_scan(const int32_t* __restrict__ sums, int64_t nT,
                                                              int64_t* __restrict__ offs, int64_t* __restrict__ total) {
  __shared__ int64_t lds[SO_THREADS / WAVE];
  so_tile_scan(sums, nT, offs, total, lds);
}

__global__ __launch_bounds__(SO_THREADS) void cn_so_atom_rank(const int32_t* __restrict__ z,
                                                              const int64_t* __restrict__ atom_ptr, int G, int64_t N,
                                                              const int64_t* __restrict__ tile_off,
                                                              int64_t* __restrict__ rank,
                                                              int64_t* __restrict__ atom_ptr_out) {
  __shared__ int lds[SO_THREADS / WAVE];
  const int64_t t0 = (int64_t)blockIdx.x * SO_TILE;
  const int64_t i0 = t0 + threadIdx.x * SO_ITEMS;
  int zz[SO_ITEMS];
  so_load4(z, i0, N, zz, 1);
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < SO_ITEMS; ++k) cnt += zz[k] != 1;
  int tot;
  int64_t r = tile_off[blockIdx.x] + so_block_scan(cnt, lds, tot);
  if (i0 > N) return;
  int g = so_first_crystal(atom_ptr, G, N, t0, i0);
#pragma unroll
  for (int k = 0; k < SO_ITEMS; ++k) {
    const int64_t i = i0 + k;
    if (i > N) break;
    while (g < G && atom_ptr[g + 1] <= i) ++g;
    if (atom_ptr[g] == i) so_store_starts(atom_ptr, atom_ptr_out, g, i, r);
    if (i < N) {
      const bool keep = zz[k] != 1;
      rank[i] = keep ? r : -1;
      r += keep;
    }
  }
}

__global__ __launch_bounds__(SO_THREADS) void cn_so_atom_fill(const int32_t* __restrict__ z,
                                                              const float* __restrict__ pos,
                                                              const int64_t* __restrict__ rank, int64_t N,
                                                              int32_t* __restrict__ z_out, float* __restrict__ pos_out,
                                                              uint8_t* __restrict__ mask_out) {
  const int64_t i0 = ((int64_t)blockIdx.x * SO_THREADS + threadIdx.x) * SO_ITEMS;
  if (i0 >= N) return;
  int zz[SO_ITEMS];
  so_load4(z, i0, N, zz, 1);
  float p[3 * SO_ITEMS];
  if (pos) {
    if (i0 + SO_ITEMS <= N) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(pos + i0 * 3 + q * 4);
        p[q * 4] = t.x; p[q * 4 + 1] = t.y; p[q * 4 + 2] = t.z; p[q * 4 + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 3 * SO_ITEMS; ++q) p[q] = i0 * 3 + q < N * 3 ? pos[i0 * 3 + q] : 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < SO_ITEMS; ++k) {
    if (i0 + k >= N || zz[k] == 1) continue;
    const int64_t r = rank[i0 + k];
    z_out[r] = zz[k];
    if (mask_out) mask_out[r] = 1;
    if (pos) {
      pos_out[r * 3] = p[k * 3];
      pos_out[r * 3 + 1] = p[k * 3 + 1];
      pos_out[r * 3 + 2] = p[k * 3 + 2];
    }
  }
}

// ---------------------------------------------------------------------------------------------------- edges
// The 4 edges i0 .. i0+3 of a thread: their crystal, whether both ends survive, and the ends' new numbers inside the
// crystal.  An end outside its crystal's atoms (a malformed shard) drops the edge and raises status 2.
struct SoEdges {
  int g[SO_ITEMS];
  int src[SO_ITEMS], tgt[SO_ITEMS];
  bool keep[SO_ITEMS];
  int count;
};

__device__ __forceinline__ void so_edges(const CartnetShard& s, int G, int64_t E, const int64_t* __restrict__ rank,
                                         const int64_t* __restrict__ atom_ptr_out, int64_t t0, int64_t i0,
                                         int64_t* __restrict__ status, SoEdges& o) {
  int src[SO_ITEMS], tgt[SO_ITEMS];
  so_load4(s.edge_src, i0, E, src, 0);
  so_load4(s.edge_tgt, i0, E, tgt, 0);
  o.count = 0;
  int g = i0 <= E ? so_first_crystal(s.edge_ptr, G, E, t0, i0) : G;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < SO_ITEMS; ++k) {
    const int64_t i = i0 + k;
    o.keep[k] = false;
    o.src[k] = o.tgt[k] = 0;
    if (i <= E)
      while (g < G && s.edge_ptr[g + 1] <= i) ++g;
    o.g[k] = g;
    if (i >= E) continue;                                    // i < E implies g < G
    const int64_t base = s.atom_ptr[g];
    const int64_t na = s.atom_ptr[g + 1] - base;
    if ((uint64_t)(int64_t)src[k] >= (uint64_t)na || (uint64_t)(int64_t)tgt[k] >= (uint64_t)na) {
      bad = true;
      continue;
    }
    const int64_t rs = rank[base + src[k]], rt = rank[base + tgt[k]];
    if (rs >= 0 && rt >= 0) {
      const int64_t nb = atom_ptr_out[g];
      o.keep[k] = true;
      o.src[k] = (int)(rs - nb);
      o.tgt[k] = (int)(rt - nb);
      ++o.count;
    }
  }
  if (bad && status) *status = 2;
}

__global__ __launch_bounds__(SO_THREADS) void cn_so_edge_count(CartnetShard s, int G, int64_t E,
                                                               const int64_t* __restrict__ rank,
                                                               const int64_t* __restrict__ atom_ptr_out,
                                                               int32_t* __restrict__ tile_sum,
                                                               int64_t* __restrict__ status) {
  __shared__ int lds[SO_THREADS / WAVE];
  const int64_t t0 = (int64_t)blockIdx.x * SO_TILE;
  SoEdges e;
  so_edges(s, G, E, rank, atom_ptr_out, t0, t0 + threadIdx.x * SO_ITEMS, status, e);
  so_block_sum_store(e.count, lds, tile_sum + blockIdx.x);
}

__global__ __launch_bounds__(SO_THREADS) void cn_so_edge_fill(CartnetShard s, int G, int64_t E,
                                                              const int64_t* __restrict__ rank,
                                                              const int64_t* __restrict__ atom_ptr_out,
                                                              const int64_t* __restrict__ tile_off,
                                                              int64_t* __restrict__ edge_ptr_out,
                                                              int32_t* __restrict__ src_out, int32_t* __restrict__ tgt_out,
                                                              float* __restrict__ dist_out, float* __restrict__ dir_out) {
  __shared__ int lds[SO_THREADS / WAVE];
  const int64_t t0 = (int64_t)blockIdx.x * SO_TILE;
  const int64_t i0 = t0 + threadIdx.x * SO_ITEMS;
  SoEdges e;
  so_edges(s, G, E, rank, atom_ptr_out, t0, i0, nullptr, e);      // count has reported a malformed shard
  float dist[SO_ITEMS], dir[3 * SO_ITEMS];
  if (i0 + SO_ITEMS <= E) {
    const f32x4 d = *reinterpret_cast<const f32x4*>(s.cart_dist + i0);
    dist[0] = d.x; dist[1] = d.y; dist[2] = d.z; dist[3] = d.w;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(s.cart_dir + i0 * 3 + q * 4);
      dir[q * 4] = t.x; dir[q * 4 + 1] = t.y; dir[q * 4 + 2] = t.z; dir[q * 4 + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < SO_ITEMS; ++k) dist[k] = i0 + k < E ? s.cart_dist[i0 + k] : 0.f;
#pragma unroll
    for (int q = 0; q < 3 * SO_ITEMS; ++q) dir[q] = i0 * 3 + q < E * 3 ? s.cart_dir[i0 * 3 + q] : 0.f;
  }
  int tot;
  int64_t r = tile_off[blockIdx.x] + so_block_scan(e.count, lds, tot);
#pragma unroll
  for (int k = 0; k < SO_ITEMS; ++k) {
    const int64_t i = i0 + k;
    if (i > E) break;
    if (s.edge_ptr[e.g[k]] == i) so_store_starts(s.edge_ptr, edge_ptr_out, e.g[k], i, r);
    if (!e.keep[k]) continue;
    src_out[r] = e.src[k];
    tgt_out[r] = e.tgt[k];
    dist_out[r] = dist[k];
    dir_out[r * 3] = dir[k * 3];
    dir_out[r * 3 + 1] = dir[k * 3 + 1];
    dir_out[r * 3 + 2] = dir[k * 3 + 2];
    ++r;
  }
}

struct SoLayout {
  int64_t nTa, nTe;
  size_t rank, sum_a, off_a, sum_e, off_e, bytes;
};

inline size_t so_align(size_t b) { return (b + 255) / 256 * 256; }

SoLayout so_layout(int64_t N, int64_t E) {
  SoLayout l;
  l.nTa = (N + 1 + SO_TILE - 1) / SO_TILE;                  // item domains are [0, N] and [0, E]
  l.nTe = (E + 1 + SO_TILE - 1) / SO_TILE;
  size_t o = 0;
  l.rank = o;  o += so_align((size_t)(N + 1) * 8);
  l.sum_a = o; o += so_align((size_t)l.nTa * 4);
  l.off_a = o; o += so_align((size_t)(l.nTa + 1) * 8);
  l.sum_e = o; o += so_align((size_t)l.nTe * 4);
  l.off_e = o; o += so_align((size_t)(l.nTe + 1) * 8);
  l.bytes = o;
  return l;
}

#define ST(s) reinterpret_cast<hipStream_t>(s)

int so_check(const CartnetShard* s, int32_t G, int64_t N, int64_t E, const void* ws, size_t ws_bytes, const char* who) {
  CN_CHECK(s, "%s: null shard", who);
  CN_CHECK(G >= 1 && N >= 0 && E >= 0, "%s: bad sizes (G=%d)", who, G);
  CN_CHECK(N < (1LL << 40) && E < (1LL << 40), "%s: shard too large for one launch", who);
  CN_CHECK(s->atom_ptr && s->edge_ptr && (N == 0 || s->z), "%s: incomplete shard", who);
  CN_CHECK(E == 0 || (s->edge_src && s->edge_tgt && s->cart_dist && s->cart_dir), "%s: edge arrays missing", who);
  CN_CHECK(ws && ws_bytes >= so_layout(N, E).bytes, "%s: workspace too small", who);
  CN_CHECK((reinterpret_cast<uintptr_t>(s->z) | reinterpret_cast<uintptr_t>(s->pos) |
            reinterpret_cast<uintptr_t>(s->edge_src) | reinterpret_cast<uintptr_t>(s->edge_tgt) |
            reinterpret_cast<uintptr_t>(s->cart_dist) | reinterpret_cast<uintptr_t>(s->cart_dir) |
            reinterpret_cast<uintptr_t>(ws)) % 16 == 0,
           "%s: arrays must be 16-byte aligned", who);
  return 0;
}

}  // namespace

extern "C" size_t cartnet_shard_drop_h_workspace_bytes(int64_t N, int64_t E) {
  if (N < 0 || E < 0) return 0;
  return so_layout(N, E).bytes;
}

extern "C" int cartnet_shard_drop_h_count(const CartnetShard* shard, int32_t G, int64_t N, int64_t E, void* workspace,
                                          size_t workspace_bytes, int64_t* atom_ptr_out, int64_t* totals,
                                          void* stream) {
  if (so_check(shard, G, N, E, workspace, workspace_bytes, "cartnet_shard_drop_h_count")) return 1;
  CN_CHECK(atom_ptr_out && totals, "cartnet_shard_drop_h_count: null output");
  const SoLayout l = so_layout(N, E);
  char* ws = static_cast<char*>(workspace);
  int64_t* rank = reinterpret_cast<int64_t*>(ws + l.rank);
  int32_t* sum_a = reinterpret_cast<int32_t*>(ws + l.sum_a);
  int64_t* off_a = reinterpret_cast<int64_t*>(ws + l.off_a);
  int32_t* sum_e = reinterpret_cast<int32_t*>(ws + l.sum_e);
  int64_t* off_e = reinterpret_cast<int64_t*>(ws + l.off_e);
  if (hipMemsetAsync(totals, 0, 3 * sizeof(int64_t), ST(stream)) != hipSuccess) {
    cartnet_set_error("cartnet_shard_drop_h_count: hipMemsetAsync failed");
    return 2;
  }
  hipLaunchKernelGGL(cn_so_atom_count, dim3((unsigned)l.nTa), dim3(SO_THREADS), 0, ST(stream), shard->z,
                     shard->non_h_mask, N, sum_a, totals + 2);
  CN_LAUNCH_CHECK("cartnet_shard_drop_h_count/atom_count");
  hipLaunchKernelGGL(cn_so_tile_scan, dim3(1), dim3(SO_THREADS), 0, ST(stream), sum_a, l.nTa, off_a, totals);
  CN_LAUNCH_CHECK("cartnet_shard_drop_h_count/atom_scan");
  hipLaunchKernelGGL(cn_so_atom_rank, dim3((unsigned)l.nTa), dim3(SO_THREADS), 0, ST(stream), shard->z, shard->atom_ptr,
                     G, N, off_a, rank, atom_ptr_out);
  CN_LAUNCH_CHECK("cartnet_shard_drop_h_count/atom_rank");
  hipLaunchKernelGGL(cn_so_edge_count, dim3((unsigned)l.nTe), dim3(SO_THREADS), 0, ST(stream), *shard, G, E, rank,
                     atom_ptr_out, sum_e, totals + 2);
  CN_LAUNCH_CHECK("cartnet_shard_drop_h_count/edge_count");
  hipLaunchKernelGGL(cn_so_tile_scan, dim3(1), dim3(SO_THREADS), 0, ST(stream), sum_e, l.nTe, off_e, totals + 1);
  CN_LAUNCH_CHECK("cartnet_shard_drop_h_count/edge_scan");
  return 0;
}

extern "C" int cartnet_shard_drop_h_fill(const CartnetShard* shard, int32_t G, int64_t N, int64_t E,
                                         const void* workspace, size_t workspace_bytes, const int64_t* atom_ptr_out,
                                         int64_t N_out, int64_t E_out, int32_t* z_out, float* pos_out,
                                         uint8_t* non_h_mask_out, int64_t* edge_ptr_out, int32_t* edge_src_out,
                                         int32_t* edge_tgt_out, float* cart_dist_out, float* cart_dir_out,
                                         void* stream) {
  if (so_check(shard, G, N, E, workspace, workspace_bytes, "cartnet_shard_drop_h_fill")) return 1;
  CN_CHECK(N_out >= 0 && N_out <= N && E_out >= 0 && E_out <= E, "cartnet_shard_drop_h_fill: bad totals");
  CN_CHECK(atom_ptr_out && edge_ptr_out, "cartnet_shard_drop_h_fill: null offsets");
  CN_CHECK(N_out == 0 || (z_out && (!shard->pos || pos_out)), "cartnet_shard_drop_h_fill: atom outputs missing");
  CN_CHECK(E_out == 0 || (edge_src_out && edge_tgt_out && cart_dist_out && cart_dir_out),
           "cartnet_shard_drop_h_fill: edge outputs missing");
  const SoLayout l = so_layout(N, E);
  const char* ws = static_cast<const char*>(workspace);
  const int64_t* rank = reinterpret_cast<const int64_t*>(ws + l.rank);
  const int64_t* off_e = reinterpret_cast<const int64_t*>(ws + l.off_e);
  if (N > 0) {
    const int64_t nb = (N + SO_TILE - 1) / SO_TILE;
    hipLaunchKernelGGL(cn_so_atom_fill, dim3((unsigned)nb), dim3(SO_THREADS), 0, ST(stream), shard->z,
                       pos_out ? shard->pos : nullptr, rank, N, z_out, pos_out, non_h_mask_out);
    CN_LAUNCH_CHECK("cartnet_shard_drop_h_fill/atoms");
  }
  hipLaunchKernelGGL(cn_so_edge_fill, dim3((unsigned)l.nTe), dim3(SO_THREADS), 0, ST(stream), *shard, G, E, rank,
                     atom_ptr_out, off_e, edge_ptr_out, edge_src_out, edge_tgt_out, cart_dist_out, cart_dir_out);
  CN_LAUNCH_CHECK("cartnet_shard_drop_h_fill/edges");
  return 0;
}

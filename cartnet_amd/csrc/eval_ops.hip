// Evaluation at any batch size with the results of batch size 1 (reference: the ADP test loader has batch size 1,
// loader/loader.py:121, so its test pass, train/train.py:202-243, averages per-crystal means, --inference, main.py:21-60,
// stores per-crystal lists, and --montecarlo, main.py:62-119, draws one rotation per crystal).  Two entry points that know
// where one crystal's rows end and the next one's begin, through a [B+1] int64 offset array on the device:
//
//   cartnet_rotate_rows  out[r] = v[r] @ R[g(r)]: the Monte-Carlo step's rotated copy of cart_dir (main.py:95), one launch
//                        for the whole batch.  g(r) by the tile / binary-search scheme of shard_tiles.h.
//   cartnet_adp_eval     per atom |pred - true| and the three metrics of cartnet_adp_metrics (adp_metrics.h: the same
//                        device function, the same bits), with the Monte-Carlo pseudo-truth R_g^T truth R_g (main.py:97)
//                        formed on the way in; per crystal the four sums the means are taken from, in fp64.
//
// No atomics, fixed summation order, fp64 sums: two runs give the same bytes.  No kernel of this unit uses scratch.
#include "common.h"
#include "adp_metrics.h"
#include "crystal_reduce.h"
#include "shard_tiles.h"

namespace {

// v' = v R as cn_collate_kernel's edge section evaluates it (collate.hip: rot_row under the default contraction compiles to
// exactly these operations -- columns 0 and 1 are two chained FMAs on the middle product, column 2 an FMA of the first two
// terms plus the separately rounded third product).  Spelled out under contract(off), where only the fmaf calls fuse (the
// _rn intrinsics are plain operators to the compiler and may be contracted), so that a copy rotated here equals
// DeviceShard.collate(sel, rot).cart_dir bit for bit (tests/test_gpu_eval_batch.py).
__device__ __forceinline__ void ev_rot_row(const float* v, const float* R, float* o) {
#pragma clang fp contract(off)
  o[0] = fmaf(v[2], R[6], fmaf(v[0], R[0], v[1] * R[3]));
  o[1] = fmaf(v[2], R[7], fmaf(v[0], R[1], v[1] * R[4]));
  const float head = fmaf(v[0], R[2], v[1] * R[5]), tail = v[2] * R[8];
  o[2] = head + tail;
}

__global__ __launch_bounds__(SO_THREADS) void cn_rotate_rows_kernel(const float* v, const int64_t* __restrict__ ptr,
                                                                    int B, int64_t n, const float* __restrict__ rot,
                                                                    float* out) {
  const int64_t t0 = (int64_t)blockIdx.x * SO_TILE, i0 = t0 + (int64_t)threadIdx.x * SO_ITEMS;
  if (i0 >= n) return;
  float a[3 * SO_ITEMS], o[3 * SO_ITEMS];
#pragma unroll
  for (int q = 0; q < 3 * SO_ITEMS; ++q) a[q] = i0 * 3 + q < n * 3 ? v[i0 * 3 + q] : 0.f;   // all reads before any write:
  int g = so_walk_first(ptr, B, n, t0, i0);                                                 // out may be v
  int loaded = -1;
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
#pragma unroll
  for (int k = 0; k < SO_ITEMS; ++k) {
    const int64_t i = i0 + k;
    if (i < n) {
      g = so_walk_to(ptr, B, g, i);                               // steps over empty segments
      if (g != loaded) {
#pragma unroll
        for (int q = 0; q < 9; ++q) R[q] = rot[(size_t)g * 9 + q];
        loaded = g;
      }
    }
    ev_rot_row(a + 3 * k, R, o + 3 * k);
  }
#pragma unroll
  for (int q = 0; q < 3 * SO_ITEMS; ++q)
    if (i0 * 3 + q < n * 3) out[i0 * 3 + q] = o[q];
}

// One workgroup per atom, as cn_adp_metrics_kernel.  Every thread holds the atom's two matrices; thread 0 writes the
// pseudo-truth and the absolute error.  The metrics are evaluated from the fp32 pseudo-truth as it is written.
__global__ __launch_bounds__(256) void cn_adp_eval_kernel(const float* __restrict__ pred, const float* __restrict__ tru,
                                                          const int64_t* __restrict__ ptr, int B, int M,
                                                          const float* __restrict__ rot, const float* __restrict__ grid,
                                                          int P, float* __restrict__ true_out,
                                                          float* __restrict__ abs_err, float* __restrict__ vol_err,
                                                          float* __restrict__ sim, float* __restrict__ iou) {
  const int a = blockIdx.x;
  float pf[9], tf[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    pf[i] = pred[(size_t)a * 9 + i];
    tf[i] = tru[(size_t)a * 9 + i];
  }
  if (rot) {                                   // R^T (t R): main.py:97, fp32, every product and sum in this order
#pragma clang fp contract(off)
    int g = so_find(ptr, 0, B + 1, (int64_t)a);
    if (g > B - 1) g = B - 1;
    float R[9], u[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = rot[(size_t)g * 9 + q];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        u[r * 3 + c] = fmaf(tf[r * 3 + 2], R[6 + c], fmaf(tf[r * 3 + 1], R[3 + c], tf[r * 3] * R[c]));
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        tf[r * 3 + c] = fmaf(R[6 + r], u[6 + c], fmaf(R[3 + r], u[3 + c], R[r] * u[c]));
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      if (true_out) true_out[(size_t)a * 9 + i] = tf[i];
      if (abs_err) abs_err[(size_t)a * 9 + i] = fabsf(pf[i] - tf[i]);
    }
  }
  if (vol_err || sim || iou) cn_adp_atom_metrics(pf, tf, a, grid, P, vol_err, sim, iou);
}

// One wave per crystal (crystal_reduce.h).  sums[g] = (sum |pred - true| over the 9 * rows elements, the nine of a row one
// after another; sum volume error, sum similarity index, sum IoU); a metric that was not computed leaves 0, a crystal
// without rows 0.
__global__ __launch_bounds__(WAVE) void cn_crystal_sums_kernel(const float* __restrict__ pred,
                                                               const float* __restrict__ tru,
                                                               const int64_t* __restrict__ ptr, int M,
                                                               const float* __restrict__ vol_err,
                                                               const float* __restrict__ sim,
                                                               const float* __restrict__ iou,
                                                               double* __restrict__ sums) {
  const int g = blockIdx.x, lane = threadIdx.x;
  int64_t r0, r1;
  cr_rows(ptr, g, M, r0, r1);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = r0 + lane; r < r1; r += WAVE) {
#pragma unroll
    for (int i = 0; i < 9; ++i) s[0] += (double)fabsf(pred[r * 9 + i] - tru[r * 9 + i]);
    if (vol_err) s[1] += (double)vol_err[r];
    if (sim) s[2] += (double)sim[r];
    if (iou) s[3] += (double)iou[r];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) s[q] = cr_wave_sum(s[q]);
  if (lane == 0)
#pragma unroll
    for (int q = 0; q < 4; ++q) sums[(size_t)g * 4 + q] = s[q];
}

}  // namespace

extern "C" int cartnet_rotate_rows(const float* v, const int64_t* row_ptr, int32_t B, int64_t n, const float* rot,
                                   float* out, void* stream) {
  CN_CHECK(B >= 1 && n >= 0, "cartnet_rotate_rows: bad sizes (B=%d, n=%lld)", B, (long long)n);
  CN_CHECK(n < (1LL << 31) * SO_TILE / 4, "cartnet_rotate_rows: too many rows for one launch");
  if (n == 0) return 0;
  CN_CHECK(v && row_ptr && rot && out, "cartnet_rotate_rows: null pointer");
  hipLaunchKernelGGL(cn_rotate_rows_kernel, dim3((unsigned)((n + SO_TILE - 1) / SO_TILE)), dim3(SO_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), v, row_ptr, B, n, rot, out);
  CN_LAUNCH_CHECK("cartnet_rotate_rows");
  return 0;
}

extern "C" int cartnet_adp_eval(const float* pred, const float* truth, const int64_t* row_ptr, int32_t B, int32_t M,
                                const float* rot, const float* grid, int32_t num_points, float* true_out, float* abs_err,
                                float* volume_error, float* similarity_index, float* iou, double* crystal_sums,
                                void* stream) {
  CN_CHECK(B >= 1 && M >= 0, "cartnet_adp_eval: bad sizes (B=%d, M=%d)", B, M);
  CN_CHECK(row_ptr && crystal_sums, "cartnet_adp_eval: row_ptr and crystal_sums are required");
  CN_CHECK(M == 0 || (pred && truth), "cartnet_adp_eval: null pointer");
  CN_CHECK(!rot || true_out, "cartnet_adp_eval: with rot the pseudo-truth needs true_out");
  CN_CHECK(!true_out || (true_out != truth && true_out != pred), "cartnet_adp_eval: true_out must not alias an input");
  CN_CHECK(!iou || (grid && num_points >= 1 && num_points <= 1024),
           "cartnet_adp_eval: the IoU needs grid[num_points], 1 <= num_points <= 1024 (got %d)", num_points);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool per_atom = true_out || abs_err || volume_error || similarity_index || iou;
  if (M > 0 && per_atom) {
    hipLaunchKernelGGL(cn_adp_eval_kernel, dim3(M), dim3(256), 0, st, pred, truth, row_ptr, B, M, rot, grid, num_points,
                       true_out, abs_err, volume_error, similarity_index, iou);
    CN_LAUNCH_CHECK("cartnet_adp_eval");
  }
  hipLaunchKernelGGL(cn_crystal_sums_kernel, dim3(B), dim3(WAVE), 0, st, pred, rot ? true_out : truth, row_ptr, M,
                     volume_error, similarity_index, iou, crystal_sums);
  CN_LAUNCH_CHECK("cartnet_adp_eval");
  return 0;
}

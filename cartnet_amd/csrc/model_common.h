// The host kit of the two step drivers (model.hip: CartNet; icomformer.hip): workspace carving, the BatchNorm-group rule,
// GEMM argument blocks, the split-K weight-gradient product with its slab check, the batcher of a step's weight forms, the
// two-stream event plumbing and the head-gradient tail.  Host code only; whatever both drivers need lives here, once.
#pragma once
#include "common.h"
#include <vector>

namespace cn_model {

constexpr int BM_TILE = 128;

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
inline int tiles_m(long long M) { return (int)((M + BM_TILE - 1) / BM_TILE); }

struct Carver {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count) {
    off = align_up(off);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
};

// BatchNorm groups inside one batch: group_count crystals-per-group blocks (1 = no grouping), and for the grouped
// statistics kernels ceil(segments / G / 4 segments-per-workgroup) partial rows per group, at most `cap`
inline int group_count(int Bg, int bn_group_size) {
  return (bn_group_size > 0 && Bg > bn_group_size) ? (Bg + bn_group_size - 1) / bn_group_size : 1;
}
inline int group_parts(size_t segments, int G, int cap) {
  const size_t per = (segments + (size_t)4 * G - 1) / ((size_t)4 * G);
  return (int)(per < 1 ? 1 : (per > (size_t)cap ? (size_t)cap : per));
}

// Split-K of the weight-gradient products: ONE workgroup per CU (256), not two.  Round 4, same-box A B A B: the step
// 14.63 / 14.92 -> 14.08 / 14.14 ms (fp32), 10.68 -> 10.59 (bf16x3), 6.55 -> 6.32 (bf16 + bf16 storage).  These launches
// live on the weight-gradient stream for the whole of backward; with 512 long-lived workgroups they took BOTH slots of
// every CU whenever the main stream's kernel retired, and every kernel of the critical chain -- above all its ~30 small
// ones -- then waited for a slot (rocprof: 5 us finalisers reading 38 us in-step).  One resident workgroup per CU runs the
// matrix pipe as well as two (0.97 of it alone, profiles/r03_exp_phases.md) and leaves the other half of every CU's
// registers to the chain that the step's length depends on.  cn_gemm_f32tn_kernel enforces it with its LDS footprint
// (four stages = 96 KB: a second one does not fit, gemm_f32.h), which is also one more K-step of prefetch.
constexpr int WGRAD_TARGET = 256;
inline int split_k(long long K, int tiles) {
  long long s = (WGRAD_TARGET + tiles - 1) / tiles;
  if (s > K / 256) s = K / 256;
  if (s < 1) s = 1;
  return (int)s;
}
inline int wgrad_tiles(int groups, int M, int N) { return groups * ((M + 127) / 128) * (N > 128 ? (N + 255) / 256 : 1); }
inline size_t wgrad_slab_floats(int groups, long long K, int M, int N) {
  const int S = split_k(K, wgrad_tiles(groups, M, N));
  return S > 1 ? (size_t)groups * S * M * N : 0;
}
#ifdef CN_HOST_PROFILE
// Diagnostic build only (tools/host_profile.py): host time of every RUN(...) statement of the sequencing code, by source
// line, summed over calls; read and reset through cartnet_debug_host_profile.  The product build has none of this.
}  // namespace cn_model
#include <chrono>
namespace cn_model {
struct HostProf { double us[4096]; long n[4096]; const char* what[4096]; };
inline HostProf& host_prof() { static HostProf p{}; return p; }
#define RUN(call)                                                                                   \
  do {                                                                                              \
    const auto _t0 = std::chrono::steady_clock::now();                                              \
    int _rc = (call);                                                                               \
    const auto _t1 = std::chrono::steady_clock::now();                                              \
    auto& _p = cn_model::host_prof();                                                               \
    _p.us[__LINE__ & 4095] += std::chrono::duration<double, std::micro>(_t1 - _t0).count();         \
    _p.n[__LINE__ & 4095] += 1;                                                                     \
    _p.what[__LINE__ & 4095] = #call;                                                               \
    if (_rc != 0) return _rc;                                                                       \
  } while (0)
#else
#define RUN(call)            \
  do {                       \
    int _rc = (call);        \
    if (_rc != 0) return _rc; \
  } while (0)
#endif

// Events that order the weight-gradient stream against the main stream (created once per thread, timing disabled).
struct EventPool {
  std::vector<hipEvent_t> ev;
  size_t next = 0;
  hipEvent_t get() {
    if (next == ev.size()) {
      hipEvent_t e;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
      ev.push_back(e);
    }
    return ev[next++];
  }
};

#ifdef CN_HOST_PROFILE
struct HostProfScope {
  int slot; const char* what; std::chrono::steady_clock::time_point t0;
  HostProfScope(int s, const char* w) : slot(s), what(w), t0(std::chrono::steady_clock::now()) {}
  ~HostProfScope() {
    auto& p = host_prof();
    p.us[slot] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    p.n[slot] += 1; p.what[slot] = what;
  }
};
#define CN_PROF_SCOPE(slot, what) cn_model::HostProfScope _scope(slot, what)
#else
#define CN_PROF_SCOPE(slot, what)
#endif
inline EventPool& event_pool() { thread_local EventPool p; return p; }      // one per thread, for both drivers

// Test-only skew of one of the two streams (cartnet_debug_stream_skew, cartnet_hip.h): which = 0 off, 1 side, 2 main.
// Off, its whole cost is one thread-local read per Streams operation; nothing is queued.
struct StreamSkew { int which = 0, usec = 0; };
inline StreamSkew& stream_skew() { thread_local StreamSkew s; return s; }

// The two streams of one entry-point call: `main` is the caller's, `side` the optional second one (the same stream, and
// every operation a no-op, when there is none).  Operations return 0, or 2 with the error text set.  The two mark_*
// return nullptr both for "one stream: nothing to order" and for a failed record; a failure is remembered, and the next
// fork / *_waits / join returns it -- a null event alone means "nothing was queued, nothing to wait for".
// With the skew on and two streams, late() queues a bounded spin (cartnet_debug_spin) on the skewed stream wherever one
// of its concurrent sections starts: in the constructor, after each of its waits, after each of its records that the other
// stream waits for -- so whatever it runs next is late against the other stream.  A spin that cannot be queued counts as
// a failed record.
struct Streams {
  const char* who;      // the entry point, for the error text
  hipStream_t main, side;
  bool dual, record_failed = false;
  EventPool* pool;
  Streams(const char* who_, void* stream, void* aux_stream)
      : who(who_), main((hipStream_t)stream), side(aux_stream ? (hipStream_t)aux_stream : (hipStream_t)stream),
        dual(aux_stream != nullptr && aux_stream != stream), pool(&event_pool()) {
    pool->next = 0;
    if (dual) late(side), late(main);
  }
  int fail(const char* what) { cartnet_set_error("%s: stream %s failed", who, what); return 2; }
  void late(hipStream_t s) {      // only called when dual
    const StreamSkew& k = stream_skew();
    if (k.which == (s == side ? 1 : 2) && cartnet_debug_spin(k.usec, (void*)s) != 0) record_failed = true;
  }
  hipEvent_t mark(hipStream_t s) {
    hipEvent_t e = pool->get();
    if (e && hipEventRecord(e, s) == hipSuccess) {
      late(s);
      return e;
    }
    record_failed = true;
    return nullptr;
  }
  int waits(hipStream_t s, hipEvent_t e, const char* what) {
    if (record_failed) return fail("event record");
    if (hipStreamWaitEvent(s, e, 0) != hipSuccess) return fail(what);
    late(s);
    return record_failed ? fail("skew spin") : 0;
  }
  // after(main) -> side waits
  int fork() {
    CN_PROF_SCOPE(4001, "Streams::fork (record + wait)");
    return dual ? waits(side, mark(main), "fork") : 0;
  }
  // the two halves of fork(), for call sites that put the main stream's next kernels in the queue BEFORE spending host
  // time on the side stream's launches (a batch of tiny crystals is host-paced: what is enqueued first starts first)
  hipEvent_t mark_main() {
    CN_PROF_SCOPE(4002, "Streams::mark_main (record)");
    return dual ? mark(main) : nullptr;
  }
  int side_waits(hipEvent_t e) {      // e comes from mark_main: null in dual mode is a failed record
    CN_PROF_SCOPE(4003, "Streams::side_waits (wait)");
    if (!dual) return 0;
    return e ? waits(side, e, "fork") : fail("fork");
  }
  hipEvent_t mark_side() {
    CN_PROF_SCOPE(4004, "Streams::mark_side (record)");
    return dual ? mark(side) : nullptr;
  }
  int main_waits(hipEvent_t e) {      // e == nullptr: nothing was queued on the side stream for this dependency
    CN_PROF_SCOPE(4005, "Streams::main_waits (wait)");
    if (!dual || (!e && !record_failed)) return 0;
    return waits(main, e, "wait");
  }
  // everything queued on the side stream precedes whatever is enqueued next on the main stream
  int join() { return main_waits(mark_side()); }
};

// ---- GEMM argument blocks ------------------------------------------------------------------------------------------------
inline CartnetGemmArgs gemm_args(int prec, int M, int N, int K, int lda, int ldb, int ldc, int tile_policy = 0) {
  CartnetGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.precision = prec;
  a.tile_policy = tile_policy;      // 1: grouped C x C products on the 128-wide fp32 kernel (CartnetGemmArgs.tile_policy)
  a.M = M; a.N = N; a.K = K;
  a.lda = lda; a.ldb = ldb; a.ldc = ldc;
  a.ngroups = 1; a.nsegs = 1; a.splitk = 1;
  return a;
}

// bytes of one [K, N] weight image at GEMM precision `prec` (images of a folded operand sit back to back)
inline size_t img_bytes(int prec, int K, int N) {
  return prec == 0 ? cartnet_gemm_pack_b_bytes(K, N) : cartnet_gemm_split_b_bytes(K, N);
}

// ---- weight gradients ----------------------------------------------------------------------------------------------------
// How a driver's weight-gradient products run: precision, tile policy and the split-K slab region of the stream they are
// queued on (`capacity` floats: the maximum of wgrad_slab_floats over the shapes the driver's carve lists).
struct WgradPlan {
  int prec, tile_policy;
  float* slabs;
  size_t capacity;
};
// outs[g] = dY[g]^T @ (silu?)(X[g]): reduction over `K` rows, split over workgroups, slabs summed in fixed order.
// dy_half / x_half: the operand is stored as bf16 (half storage).
inline int wgrad(const WgradPlan& p, const float* const* dY, int ldy, const float* const* X, int ldx, float* const* outs,
                 int ldo, long long K, int M, int N, int groups, bool b_act, void* st, bool dy_half = false,
                 bool x_half = false) {
  if (K <= 0) {   // no rows: the gradient is zero
    for (int g = 0; g < groups; ++g)
      for (int r = 0; r < M; ++r)
        if (hipMemsetAsync(outs[g] + (size_t)r * ldo, 0, sizeof(float) * N, (hipStream_t)st) != hipSuccess) return 2;
    return 0;
  }
  const int S = split_k(K, wgrad_tiles(groups, M, N));
  const size_t need = wgrad_slab_floats(groups, K, M, N);
  CN_CHECK(need <= p.capacity,
           "wgrad: %d x [%d, %d] over K = %lld needs %zu slab floats, %zu were carved (the shape is missing from the carve list)",
           groups, M, N, K, need, p.capacity);
  CartnetGemmArgs a = gemm_args(p.prec, M, N, (int)K, ldy, ldx, S > 1 ? N : ldo, p.tile_policy);
  a.ngroups = groups; a.a_kstrided = 1; a.b_kstrided = 1; a.splitk = S;
  a.b_act = b_act ? 1 : 0; a.a_half = dy_half ? 1 : 0; a.b_half = x_half ? 1 : 0;
  const float* slabp[CARTNET_MAX_GROUPS];
  for (int g = 0; g < groups; ++g) {
    a.A[g] = dY[g];
    a.B[g] = X[g];
    a.C[g] = S > 1 ? p.slabs + (size_t)g * S * M * N : outs[g];
    slabp[g] = a.C[g];
  }
  RUN(cartnet_gemm(&a, st));
  if (S > 1) RUN(cartnet_splitk_reduce(slabp, outs, groups, S, M, N, ldo, st));
  return 0;
}

// ---- weight forms of a step ----------------------------------------------------------------------------------------------
// The transposed copies and pre-arranged images of a step's weights, collected and launched in batches.  One per thread
// (weight_forms()); the vectors keep their capacity, so after a thread's first call nothing here touches the heap.
struct WeightForms {
  std::vector<const float*> isrc, tsrc;
  std::vector<void*> idst;
  std::vector<float*> tdst;
  std::vector<int32_t> iK, iN, isk, isn, trows, tcols, tlds, tldd;
  void clear() {
    isrc.clear(); idst.clear(); iK.clear(); iN.clear(); isk.clear(); isn.clear();
    tsrc.clear(); tdst.clear(); trows.clear(); tcols.clear(); tlds.clear(); tldd.clear();
  }
  // image of the operand B[k, n] = src[k * stride_k + n * stride_n]  (W^T of a row-major W: strides 1, ld; W itself: ld, 1)
  void image(const float* src, void* dst, int K, int N, int stride_k, int stride_n) {
    isrc.push_back(src); idst.push_back(dst); iK.push_back(K); iN.push_back(N); isk.push_back(stride_k); isn.push_back(stride_n);
  }
  void transpose(const float* src, float* dst, int rows, int cols, int lds, int ldd) {
    tsrc.push_back(src); tdst.push_back(dst); trows.push_back(rows); tcols.push_back(cols); tlds.push_back(lds); tldd.push_back(ldd);
  }
  int flush_transposes(void* st) {
    constexpr size_t TB = 40;   // cartnet_transpose takes up to 40 matrices per launch
    for (size_t j = 0; j < tsrc.size(); j += TB)
      RUN(cartnet_transpose(tsrc.data() + j, tdst.data() + j, trows.data() + j, tcols.data() + j, tlds.data() + j,
                            tldd.data() + j, (int)(tsrc.size() - j < TB ? tsrc.size() - j : TB), st));
    return 0;
  }
  int flush_images(int prec, void* st) {      // fp32 rows at precision 0, bf16 planes at precision 1 / 2
    if (isrc.empty()) return 0;
    return (prec == 0 ? cartnet_gemm_pack_b : cartnet_gemm_split_b)(isrc.data(), idst.data(), iK.data(), iN.data(), isk.data(),
                                                                   isn.data(), (int32_t)isrc.size(), st);
  }
};
inline WeightForms& weight_forms() { thread_local WeightForms f; return f; }

// ---- head gradient -------------------------------------------------------------------------------------------------------
// The head's backward kernel leaves partial rows [nw2 | nb2, padded to 8 | H]: dW of the second Linear, its bias gradient,
// the bias gradient of the first.  Cholesky head: (6H, 6); scalar head: (H, 1).  Sums them and copies the three pieces out.
inline int head_grad_tail(const char* who, const float* head_parts, int nparts, float* head_tot, int nw2, int nb2, int H,
                          float* head2_w, float* head2_b, float* head0_b, void* st) {
  RUN(cartnet_colsum_finalize_f32(head_parts, nparts, nw2 + 8 + H, head_tot, st));
  hipStream_t s = (hipStream_t)st;
  if (hipMemcpyAsync(head2_w, head_tot, sizeof(float) * nw2, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(head2_b, head_tot + nw2, sizeof(float) * nb2, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(head0_b, head_tot + nw2 + 8, sizeof(float) * H, hipMemcpyDeviceToDevice, s) != hipSuccess) {
    cartnet_set_error("%s: head gradient copy failed", who);
    return 2;
  }
  return 0;
}

}  // namespace cn_model


// The stream-order test seam (cartnet_hip.h: cartnet_debug_spin, cartnet_debug_stream_skew): a bounded delay kernel and
// the per-thread switch that makes Streams (model_common.h) queue it on one of a call's two streams.  Off by default.
#include "model_common.h"

namespace {
constexpr int SPIN_MAX_USEC = 5000;
// The loop's second bound.  One iteration is a clock read and an s_sleep of 8 x 64 cycles (0.2 us at 2.4 GHz, a few us
// at the lowest shader clock): 5000 us take some 25,000 iterations, and 1 << 18 of them end within a second at any
// clock the chip runs at, whatever the wall clock reads.
constexpr int SPIN_MAX_ITERS = 1 << 18;

__global__ void cn_debug_spin_kernel(long long ticks) {
  const long long t0 = (long long)wall_clock64();
  for (int i = 0; i < SPIN_MAX_ITERS; ++i) {
    if ((long long)wall_clock64() - t0 >= ticks) break;
    __builtin_amdgcn_s_sleep(8);
  }
}
}  // namespace

extern "C" int cartnet_debug_spin(int32_t usec, void* stream) {
  CN_CHECK(usec >= 0 && usec <= SPIN_MAX_USEC, "cartnet_debug_spin: usec = %d is outside 0..%d", usec, SPIN_MAX_USEC);
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess ||
      khz <= 0) {
    cartnet_set_error("cartnet_debug_spin: the device reports no wall clock rate");
    return 2;
  }
  const long long ticks = ((long long)usec * khz + 999) / 1000;      // rounded up: never shorter than asked
  hipLaunchKernelGGL(cn_debug_spin_kernel, dim3(1), dim3(1), 0, reinterpret_cast<hipStream_t>(stream), ticks);
  CN_LAUNCH_CHECK("cartnet_debug_spin");
  return 0;
}

extern "C" int cartnet_debug_stream_skew(int32_t which, int32_t usec) {
  CN_CHECK(which >= 0 && which <= 2, "cartnet_debug_stream_skew: which = %d is not 0 (off), 1 (side) or 2 (main)", which);
  CN_CHECK(usec >= 0 && usec <= SPIN_MAX_USEC, "cartnet_debug_stream_skew: usec = %d is outside 0..%d", usec, SPIN_MAX_USEC);
  cn_model::StreamSkew& k = cn_model::stream_skew();
  k.which = which;
  k.usec = which ? usec : 0;
  return 0;
}

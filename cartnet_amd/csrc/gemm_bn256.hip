// Instantiations of the fp32 MFMA GEMM for 256-column output tiles (split per tile width to compile in parallel), and the
// weight-gradient launcher of the DMA-fed kernels with its K-tail kernel.
#include "gemm_kernel.h"

namespace cn_gemm {
template void launch_bn<256>(const CartnetGemmArgs&, const GemmFlags&, bool, hipStream_t);

// precision 0: the all-DMA fp32 kernel (gemm_f32.h); precision 1 / 2: the transposing-read kernel (gemm_x3.h).  Every row
// tile (a ragged last one too: M % 4 == 0, its lanes clamp) over the whole K-steps; a K tail (< 16 rows, split-K only) is
// one more slab.  (SiLU on the B operand: the five-stage fp32 instance that activates its DMA'd tiles in place in LDS,
// gemm_f32.h -- 10 % slower than a plain operand; on the fragments it was 15 % and the register-staged kernel 2-3x.)
void launch_tn(const CartnetGemmArgs& a, GemmFlags fl, hipStream_t st) {
  const int K16 = (a.K / BK) * BK, tail = a.K - K16;
  const int nfast = tail ? a.splitk - 1 : a.splitk;
  const dim3 grid(cn_ceil_div(a.M, BM) * (a.N / 256), nfast, a.ngroups);
  fl.tile_m0 = 0; fl.split0 = 0; fl.k_lo = 0; fl.k_hi = K16;
  fl.kchunk = cn_ceil_div(cn_ceil_div(K16, nfast), BK) * BK;
  if (fl.x3) launch_x3tn(a.b_act, a, fl, grid, st);
  else launch_f32tn(a.b_act, a, fl, grid, st);
  if (tail) {
    const long long items = (long long)a.M * (a.N / 4);
    const int blocks = (int)(items / 256 + 1 > 2048 ? 2048 : items / 256 + 1);
    if (a.b_act) hipLaunchKernelGGL((cn_gemm_tn_tail_kernel<true>), dim3(blocks, a.ngroups), dim3(256), 0, st, a, K16, nfast);
    else hipLaunchKernelGGL((cn_gemm_tn_tail_kernel<false>), dim3(blocks, a.ngroups), dim3(256), 0, st, a, K16, nfast);
  }
}
}  // namespace cn_gemm

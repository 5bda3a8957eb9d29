// Instantiations of the fp32 MFMA GEMM for 128-column output tiles (split per tile width to compile in parallel).
#include "gemm_kernel.h"

namespace cn_gemm {
template void launch_bn<128>(const CartnetGemmArgs&, const GemmFlags&, bool, hipStream_t);
}

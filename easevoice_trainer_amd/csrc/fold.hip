// fold_partials: second stage of the reductions whose output is tiny and whose input is long -- the weight gradients of
// the Cout = 1 / Cin = 1 layers and of the 16- / 32-channel vocoder stages (src/easevoice/module/models.py:419-446,
// 490-497, 536, 566-574 through torch.autograd).  Hundreds of blocks each hold a partial copy of a 0.2 - 12 KB result.
// Added with fp32 atomics, every address takes one atomic per block, and same-address atomics from different XCDs
// serialise at the memory side (~50 ns each: 256 blocks = 13 us per launch whatever the kernel did before, and an order
// of additions that changes from run to run).  Instead: every block stores its partial in a scratch row, and this kernel
// adds the rows in a fixed order:  out[e] += sum_b part[b * stride + e].  A row may end with a second, short result (the
// bias sums behind a weight-gradient image): elements n .. n + n2 of the row go to out2, in the same launch.
//   block = 16 consecutive outputs x 16 row groups; a thread adds rows g, g + 16, g + 32, ... (8 loads in flight), the 16
//   groups meet in LDS and are added in index order.  256 rows of 3072 floats: 192 blocks, two round trips per thread.
#include "conv_p.h"

namespace evt_conv {
namespace {

__global__ __launch_bounds__(256) void fold_partials(const float* part, long stride, int nb, float* out, long n,
                                                     float* out2, long n2) {
  __shared__ float red[16][17];
  const int el = threadIdx.x & 15, g = threadIdx.x >> 4;
  const long e = (long)blockIdx.x * 16 + el;
  float s = 0.f;
  if (e < n + n2) {
    int b = g;
    for (; b + 7 * 16 < nb; b += 8 * 16) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = part[(long)(b + u * 16) * stride + e];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; b < nb; b += 16) s += part[(long)b * stride + e];
  }
  red[g][el] = s;
  __syncthreads();
  if (g == 0 && e < n + n2) {
    float v = red[0][el];
#pragma unroll
    for (int k = 1; k < 16; ++k) v += red[k][el];
    if (e < n) out[e] += v;
    else out2[e - n] += v;
  }
}

}  // namespace

int launch_fold_partials2(const float* part, long stride, int nb, float* out, long n, float* out2, long n2,
                          hipStream_t st) {
  if (!part || !out || nb <= 0 || n <= 0 || n2 < 0 || (n2 > 0 && !out2)) return EVT_EINVAL;
  hipLaunchKernelGGL(fold_partials, dim3((unsigned)((n + n2 + 15) / 16)), dim3(256), 0, st, part, stride, nb, out, n, out2,
                     n2);
  return evt_check_launch();
}

int launch_fold_partials(const float* part, long stride, int nb, float* out, long n, hipStream_t st) {
  return launch_fold_partials2(part, stride, nb, out, n, nullptr, 0, st);
}

}  // namespace evt_conv

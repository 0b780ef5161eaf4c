// The audio slicer's arithmetic (src/audiokit/slicer/slicer.py:149-180 and src/service/audio.py:172-178 of the reference)
// for a ragged batch of recordings that live in ONE packed fp32 buffer: recording r is x[off[r] : off[r] + len[r]].
//   * evt_rms_frames_rows: get_rms -- sqrt(mean(v * v)) over a window of `win` samples every `hop` samples, the window
//     centred (zeros outside the recording) -- with the `win` additions in the order NumPy's pairwise float32 summation of a
//     contiguous run takes them, so that a frame equals the reference's bit for bit and every `rms < threshold` / argmin of
//     the host's tag walk decides as the reference does;
//   * evt_span_peak_rows: max |x| over spans of the buffer (the recordings, then the chunks), NaN propagating;
//   * evt_slice_pack_rows: the per-chunk rescale in numpy's float32 steps, cast to int16 and packed.
// dtype-independent: fp32 in, fp32 / int16 out.  No host synchronisation anywhere.
//
// The summation tree depends on `win` alone.  The host (the entry point below) cuts [0, win) into leaves of at most 128
// values as the recursion n2 = n / 2, n2 -= n2 % 8 does and lists the additions that join them; the kernel gets both by
// value.  One wave owns one frame; a lane owns a (leaf, accumulator) pair: accumulator j of a leaf adds the leaf's values
// j, j + 8, j + 16, ... in ascending order, the eight are joined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) by the
// xor butterfly 1, 2, 4 (fp32 addition commutes, so every lane of the eight holds that value), lane j = 0 adds the
// n % 8 leftovers one by one.  The samples are read from global memory directly: the eight lanes of a leaf read 32
// consecutive bytes, a sample is read by win / hop (4 at the defaults) frames and those reads hit the cache; staging a span
// in LDS would put the lanes of a thread-per-frame layout on one bank at hop = 320 = 5 * 64 and buys nothing here -- the
// whole pass is a few hundred MB per hour of audio.
#include "evt_common.h"
#include "../../include/evt.h"

namespace {

constexpr int kRmsMaxWin = 8192;    // window lengths served
constexpr int kRmsMaxLeaf = 128;    // leaves of the summation tree (a window of 8192 has 64; odd lengths a few more)
constexpr int kRmsWaves = 4;        // frames per block

// node numbering: leaf l is node l, addition c is node kRmsMaxLeaf + c = node a[c] + node b[c]; the last addition is the sum
struct RmsPlan {
  int16_t start[kRmsMaxLeaf];
  uint8_t n[kRmsMaxLeaf];           // 1 .. 128
  uint8_t a[kRmsMaxLeaf], b[kRmsMaxLeaf];
  int32_t nleaf, ncomb;
};

// numpy's pairwise_sum recursion over [start, start + n): returns the node that holds the sum, -1 when the plan is full
int plan_build(RmsPlan& p, int start, int n) {
  if (n <= 128) {
    if (p.nleaf >= kRmsMaxLeaf) return -1;
    p.start[p.nleaf] = (int16_t)start;
    p.n[p.nleaf] = (uint8_t)n;
    return p.nleaf++;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  const int l = plan_build(p, start, n2);
  const int r = l < 0 ? -1 : plan_build(p, start + n2, n - n2);
  if (r < 0 || p.ncomb >= kRmsMaxLeaf - 1) return -1;
  p.a[p.ncomb] = (uint8_t)l;
  p.b[p.ncomb] = (uint8_t)r;
  return kRmsMaxLeaf + p.ncomb++;
}

__global__ __launch_bounds__(64 * kRmsWaves) void rms_frames_kernel(const float* __restrict__ x, long x_len,
                                                                    const int64_t* __restrict__ off,
                                                                    const int64_t* __restrict__ len, int nrec, int win, int hop,
                                                                    const RmsPlan plan, const int64_t* __restrict__ frame_off,
                                                                    long total, float* __restrict__ rms) {
  // a product and the addition behind it stay two roundings: plain operators under this pragma (the __fmul_rn / __fadd_rn of
  // the HIP headers are plain operators compiled outside it, and a pair of them is contracted into an fma)
#pragma clang fp contract(off)
  __shared__ float node[kRmsWaves][2 * kRmsMaxLeaf];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long g = (long)blockIdx.x * kRmsWaves + wave;
  bool live = g < total;
  long base = 0, n_r = 0, p0 = 0;
  if (live) {
    int lo = 0, hi = nrec;              // frame_off[lo] <= g < frame_off[hi]: the recording this frame belongs to
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (frame_off[mid] <= g) lo = mid; else hi = mid;
    }
    const long f = g - frame_off[lo];
    base = off[lo];
    n_r = len[lo];
    // a table that does not describe the buffer is refused here: nothing outside [off, off + len) of x is ever read
    live = f >= 0 && n_r >= 1 && base >= 0 && base <= x_len - n_r && f < (n_r + 2 * (win / 2) - win) / hop + 1;
    p0 = f * hop - win / 2;
  }
  const float* xr = x + base;
  auto sq = [&](int k) -> float {
#pragma clang fp contract(off)
    const long p = p0 + k;
    const float v = (live && p >= 0 && p < n_r) ? xr[p] : 0.f;
    return v * v;
  };
  const int nleaf = min(max(plan.nleaf, 1), kRmsMaxLeaf);
  for (int q = lane; q < ((nleaf * 8 + 63) & ~63); q += 64) {
    const int leaf = q >> 3, j = q & 7;
    const bool act = leaf < nleaf;
    // clamped into the window, whatever the plan says
    const int st = act ? min(max((int)plan.start[leaf], 0), win) : 0;
    const int n = act ? min((int)plan.n[leaf], win - st) : 0;
    const int m = n - (n & 7);
    float acc = 0.f;
    if (n >= 8) {
      acc = sq(st + j);
      for (int i = 8; i < m; i += 8) acc = acc + sq(st + i + j);
    }
    acc = __fadd_rn(acc, __shfl_xor(acc, 1, 64));
    acc = __fadd_rn(acc, __shfl_xor(acc, 2, 64));
    acc = __fadd_rn(acc, __shfl_xor(acc, 4, 64));
    if (act && j == 0) {
      float res = n >= 8 ? acc : 0.f;
      for (int i = n >= 8 ? m : 0; i < n; ++i) res = res + sq(st + i);
      node[wave][leaf] = res;
    }
  }
  __syncthreads();
  if (lane == 0 && live) {
    const int ncomb = min(max(plan.ncomb, 0), kRmsMaxLeaf - 1);
    float* nd = node[wave];
    for (int c = 0; c < ncomb; ++c) nd[kRmsMaxLeaf + c] = __fadd_rn(nd[plan.a[c]], nd[plan.b[c]]);
    const float sum = ncomb ? nd[kRmsMaxLeaf + ncomb - 1] : nd[0];
    // sqrtf and the division are correctly rounded in this build (hipcc's default); __fsqrt_rn is the native
    // instruction, 1 ulp
    rms[g] = sqrtf(sum / (float)win);
  }
}

// a span of the buffer, or nothing where the table does not describe it
__device__ __forceinline__ long span_count(long base, long cnt, long x_len) {
  return (base >= 0 && cnt > 0 && base <= x_len - cnt) ? cnt : 0;
}

// max |x| on the bit patterns: without its sign an fp32 orders as an unsigned integer, and every NaN lies above infinity,
// so a NaN anywhere in the span makes the peak a NaN (as np.abs(x).max()).  peak is zeroed in front of the launch.
__global__ __launch_bounds__(256) void span_peak_kernel(const float* __restrict__ x, long x_len,
                                                        const int64_t* __restrict__ src_off, const int64_t* __restrict__ n,
                                                        unsigned* __restrict__ peak) {
  const int s = blockIdx.y;
  const long base = src_off[s];
  const long cnt = span_count(base, n[s], x_len);
  unsigned m = 0;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < cnt; i += gridDim.x * 256L)
    m = max(m, __float_as_uint(x[base + i]) & 0x7fffffffu);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(&peak[s], m);
}

// audio.py:172-178 per sample, every operation rounded to fp32 on its own
__global__ __launch_bounds__(256) void slice_pack_kernel(const float* __restrict__ x, long x_len,
                                                         const int64_t* __restrict__ src_off, const int64_t* __restrict__ n,
                                                         const int64_t* __restrict__ dst_off, const float* __restrict__ peak,
                                                         float c1, float c2, int16_t* __restrict__ out, long out_len) {
#pragma clang fp contract(off)
  const int s = blockIdx.y;
  const long base = src_off[s], dst = dst_off[s];
  long cnt = span_count(base, n[s], x_len);
  if (dst < 0 || dst > out_len - cnt) cnt = 0;
  const float pk = peak[s];
  for (long i = blockIdx.x * 256L + threadIdx.x; i < cnt; i += gridDim.x * 256L) {
    float v = x[base + i];
    if (pk > 1.f) v = __fdiv_rn(v, pk);
    const float w = rescale_one(v, pk, c1, c2);
    out[dst + i] = pk == 0.f ? (int16_t)0 : trunc_s16(__fmul_rn(w, 32767.f));
  }
}

// blocks along a span: eight samples a thread, at most 2048 (the kernels stride over what is left)
inline unsigned span_blocks(int64_t max_n) { return (unsigned)min((int64_t)2048, max((int64_t)1, (max_n + 2047) / 2048)); }

}  // namespace

extern "C" {

int evt_rms_frames_rows(const float* x, int64_t x_len, const int64_t* off, const int64_t* len, int32_t nrec, int32_t win,
                        int32_t hop, float* rms, const int64_t* frame_off, int64_t total_frames, void* stream) {
  if (!x || !off || !len || !rms || !frame_off || x_len <= 0 || nrec <= 0 || win <= 0 || hop <= 0 || total_frames <= 0 ||
      total_frames > 0x7fffffffLL * kRmsWaves)
    return EVT_EINVAL;
  if (win > kRmsMaxWin) return EVT_ENOTSUP;
  RmsPlan plan = {};
  if (plan_build(plan, 0, win) < 0) return EVT_ENOTSUP;
  hipLaunchKernelGGL(rms_frames_kernel, dim3((unsigned)((total_frames + kRmsWaves - 1) / kRmsWaves)), dim3(64 * kRmsWaves), 0,
                     (hipStream_t)stream, x, (long)x_len, off, len, nrec, win, hop, plan, frame_off, (long)total_frames, rms);
  return evt_check_launch();
}

int evt_span_peak_rows(const float* x, int64_t x_len, const int64_t* src_off, const int64_t* n, int32_t nspan, int64_t max_n,
                       float* peak, void* stream) {
  if (!x || !src_off || !n || !peak || x_len <= 0 || nspan <= 0 || nspan > 65535 || max_n < 0) return EVT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(peak, 0, sizeof(float) * (size_t)nspan, st) != hipSuccess) return EVT_ELAUNCH;
  hipLaunchKernelGGL(span_peak_kernel, dim3(span_blocks(max_n), nspan), dim3(256), 0, st, x, (long)x_len, src_off, n,
                     reinterpret_cast<unsigned*>(peak));
  return evt_check_launch();
}

int evt_slice_pack_rows(const float* x, int64_t x_len, const int64_t* src_off, const int64_t* n, const int64_t* dst_off,
                        const float* peak, float c1, float c2, int32_t nspan, int64_t max_n, int16_t* out, int64_t out_len,
                        void* stream) {
  if (!x || !src_off || !n || !dst_off || !peak || !out || x_len <= 0 || out_len <= 0 || nspan <= 0 || nspan > 65535 ||
      max_n < 0)
    return EVT_EINVAL;
  hipLaunchKernelGGL(slice_pack_kernel, dim3(span_blocks(max_n), nspan), dim3(256), 0, (hipStream_t)stream, x, (long)x_len,
                     src_off, n, dst_off, peak, c1, c2, out, (long)out_len);
  return evt_check_launch();
}

}  // extern "C"

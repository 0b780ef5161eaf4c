// Element-wise / normalisation kernels of the feature extractors that produce the training set's 3-bert/*.pt and
// 4-cnhubert/*.pt (src/normalization/normalize.py:88-106,132-180 of the reference, which runs
// transformers' BertForMaskedLM and HubertModel on the CPU).  The transformer layers of both models run on the library's
// convolution / attention / LayerNorm kernels; what those models need beyond them is here:
//   * GELU (erf form: transformers' "gelu" activation of both models), with an optional bias row added first and an
//     optional time-axis trim -- the tail of HuBERT's positional convolution (HubertPositionalConvEmbedding: conv with
//     padding k/2, drop the last frame of an even kernel, GELU) is ONE launch;
//   * per-channel normalisation over time + GELU: HuBERT's first feature-extractor layer (GroupNorm with one channel per
//     group, "feat_extract_norm": "group", then GELU) -- statistics per (item, channel) over all frames, two passes for
//     the variance (a 10 s clip has 32 000 frames: E[x^2] - E[x]^2 in fp32 would lose the variance of a near-constant
//     channel);
//   * the same layer for a RAGGED batch of clips with the convolution in front of it folded in (evt_hubert_front_rows:
//     conv 1 -> 512, k 10, stride 5 recomputed in each of three passes instead of stored, per-row frame counts, partial
//     sums per chunk of frames in a fixed order so that a row does not depend on the batch it is in);
//   * the clip rescaling of the `ssl` step for a ragged batch (evt_clip_rescale_rows: peak, the float clip for HuBERT and
//     the int16 clip for 5-wav32k, numpy's float32 arithmetic operation for operation).
// Inference only: forward launches, no saved statistics.  HBM-bound streams: 16-byte accesses along the channel axis.
#include "evt_common.h"
#include "../../include/evt.h"

namespace {

__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

// out[b][t][c] = gelu(x[b][t][c] + bias[c]) for t < t_out <= t_in (rows t >= t_out of the input are dropped)
template <typename T>
__global__ void gelu_rows_kernel(const T* x, const float* bias, T* out, long nseq, int t_in, int t_out, int C) {
  const long n = nseq * (long)t_out * C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long row = i / C;
    const int c = (int)(i - row * C);
    const long b = row / t_out;
    const long t = row - b * t_out;
    const float v = to_f<T>(x[(b * t_in + t) * C + c]) + (bias ? bias[c] : 0.f);
    out[i] = from_f<T>(gelu_f(v));
  }
}

// one block per (item, 64 channels): lane = channel, the four waves stride over the frames
template <typename T>
__global__ __launch_bounds__(256) void channel_norm_gelu_kernel(const T* x, const float* gamma, const float* beta, float eps,
                                                                T* out, int Tn, int C, int gelu) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + lane;
  const bool live = c < C;
  const T* xb = x + (long)blockIdx.x * Tn * C;
  T* ob = out + (long)blockIdx.x * Tn * C;
  float s = 0.f;
  if (live)
    for (int t = wave; t < Tn; t += 4) s += to_f<T>(xb[(long)t * C + c]);
  red[wave][lane] = s;
  __syncthreads();
  const float mean = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (float)Tn;
  __syncthreads();
  float q = 0.f;
  if (live)
    for (int t = wave; t < Tn; t += 4) {
      const float d = to_f<T>(xb[(long)t * C + c]) - mean;
      q += d * d;
    }
  red[wave][lane] = q;
  __syncthreads();
  const float var = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (float)Tn;     // biased, as GroupNorm
  const float rstd = rsqrtf(var + eps);
  if (!live) return;
  const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
  for (int t = wave; t < Tn; t += 4) {
    const float v = (to_f<T>(xb[(long)t * C + c]) - mean) * rstd * g + bt;
    ob[(long)t * C + c] = from_f<T>(gelu ? gelu_f(v) : v);
  }
}

inline int ew_blocks(long n) {
  long b = (n + 255) / 256;
  return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}

// ---- HuBERT's first layer on a ragged batch: conv(1 -> 512, k 10, s 5) + GroupNorm(512, 512) + GELU, the convolution
// never stored.  A block owns kFChunk consecutive frames of ONE row, counted from the row's frame 0, for all 512 channels:
// lane l of every wave holds the 80 weights of channels 8 l .. 8 l + 7 in registers (staged through LDS so that the 20 KB
// are read from memory coalesced, once per block), the four waves take the chunk's frames v, v + 4, ..., and the samples
// of the chunk (5 * frames + 5 floats) are read from LDS as wave-wide broadcasts.  Three passes over the same staged data
// compute the same fma chain, so the value that is normalised is bit for bit the value the statistics were taken from.
constexpr int kFC = 512, kFK = 10, kFS = 5;
constexpr int kFChunk = EVT_HUBERT_FRONT_CHUNK;
constexpr int kFSpan = kFChunk * kFS + (kFK - kFS);
constexpr int kFWRow = kFC + 4;    // LDS row of one tap: 516 floats keep the rows 16-byte aligned and the staging stores
                                   // (lane -> (channel, tap) = (i / 10, i % 10), bank 4 tap + channel) at most 2-way

__device__ __forceinline__ int front_frames(int n) { return n < kFK ? 0 : (n - kFK) / kFS + 1; }

enum { kFrontSum = 1, kFrontSq = 2, kFrontStore = 3 };

template <typename T> __device__ __forceinline__ void store8(T* p, const float* v);
template <> __device__ __forceinline__ void store8<float>(float* p, const float* v) {
  reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}
template <> __device__ __forceinline__ void store8<h16_t>(h16_t* p, const float* v) {
  *reinterpret_cast<uint4*>(p) = make_uint4(f2h_pack(v[0], v[1]), f2h_pack(v[2], v[3]), f2h_pack(v[4], v[5]),
                                            f2h_pack(v[6], v[7]));
}

// grid (chunks of the longest possible row, nseq), 256 threads.  part [nseq][nchunk][512]: kFrontSum / kFrontSq write the
// chunk's channel sums (of c / of (c - mean)^2) there; blocks behind a row's last frame write nothing (the statistics
// kernel reads only the row's own chunks) and, in kFrontStore, store the zero tail.
template <typename T, int PASS>
__global__ __launch_bounds__(256, 3) void hubert_front_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens,
                                                           int N, int T1, int nchunk, const float* __restrict__ w,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           float* __restrict__ part, T* __restrict__ out) {
  __shared__ __align__(16) float wl[kFK * kFWRow];
  __shared__ float xs[kFSpan];
  __shared__ float red[PASS == kFrontStore ? 1 : 4][PASS == kFrontStore ? 1 : kFC];
  const int s = blockIdx.y, chunk = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = lane * 8;
  const int Ts = front_frames(min(max(lens[s], 0), N));
  const int t0 = chunk * kFChunk;
  const int tl = min(kFChunk, Ts - t0);              // live frames of this chunk (block-uniform; <= 0: none)
  const int tw = min(kFChunk, T1 - t0);              // frames of this chunk that exist in `out`
  T* ob = PASS == kFrontStore ? out + ((long)s * T1 + t0) * kFC + c0 : nullptr;
  if (PASS == kFrontStore) {
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int f = max(tl, 0) + wave; f < tw; f += 4) store8<T>(ob + (long)f * kFC, z);
  }
  if (tl <= 0) return;
  for (int i = threadIdx.x; i < kFC * kFK; i += 256) wl[(i % kFK) * kFWRow + i / kFK] = w[i];
  // samples 5 t0 .. 5 (t0 + tl - 1) + 9 <= 5 (Ts - 1) + 9 < n_s: nothing at or behind the row's end is read
  const float* xr = wav + (long)s * N + (long)t0 * kFS;
  for (int i = threadIdx.x; i < tl * kFS + (kFK - kFS); i += 256) xs[i] = xr[i];
  __syncthreads();
  float wr[kFK][8];
#pragma unroll
  for (int j = 0; j < kFK; ++j) {
    const float4 a = *reinterpret_cast<const float4*>(&wl[j * kFWRow + c0]);
    const float4 b = *reinterpret_cast<const float4*>(&wl[j * kFWRow + c0 + 4]);
    wr[j][0] = a.x, wr[j][1] = a.y, wr[j][2] = a.z, wr[j][3] = a.w;
    wr[j][4] = b.x, wr[j][5] = b.y, wr[j][6] = b.z, wr[j][7] = b.w;
  }
  float m[8], r[8], g[8], bt[8], acc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    acc[c] = 0.f;
    m[c] = PASS != kFrontSum ? mean[(long)s * kFC + c0 + c] : 0.f;
    r[c] = PASS == kFrontStore ? rstd[(long)s * kFC + c0 + c] : 0.f;
    g[c] = PASS == kFrontStore ? gamma[c0 + c] : 0.f;
    bt[c] = PASS == kFrontStore ? beta[c0 + c] : 0.f;
  }
  for (int f = wave; f < tl; f += 4) {
    float xv[kFK], cv[8];
#pragma unroll
    for (int j = 0; j < kFK; ++j) xv[j] = xs[f * kFS + j];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < kFK; ++j) a = fmaf(wr[j][c], xv[j], a);
      cv[c] = a;
    }
    if (PASS == kFrontSum) {
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] += cv[c];
    } else if (PASS == kFrontSq) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float d = cv[c] - m[c];
        acc[c] = fmaf(d, d, acc[c]);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        cv[c] = gelu_f((cv[c] - m[c]) * r[c] * g[c] + bt[c]);
        // one erf at a time: interleaved, the eight polynomial evaluations take ~390 registers (one wave per SIMD)
        __builtin_amdgcn_sched_barrier(0);
      }
      store8<T>(ob + (long)f * kFC, cv);
    }
  }
  if (PASS != kFrontStore) {
#pragma unroll
    for (int c = 0; c < 8; ++c) red[wave][c0 + c] = acc[c];
    __syncthreads();
    float* pp = part + ((long)s * nchunk + chunk) * kFC;
    for (int ch = threadIdx.x; ch < kFC; ch += 256) pp[ch] = (red[0][ch] + red[1][ch]) + (red[2][ch] + red[3][ch]);
  }
}

// grid (2, nseq), 256 threads: thread = channel.  dst[s][ch] = sum of the row's chunk partials in ascending chunk order
// over T_s (mode 0: the mean), or rsqrt(that + eps) (mode 1: from the squared deviations); 0 for a row without frames.
__global__ __launch_bounds__(256) void hubert_front_stat_kernel(const float* __restrict__ part,
                                                                const int32_t* __restrict__ lens, int N, int nchunk,
                                                                float eps, int mode, float* __restrict__ dst) {
  const int s = blockIdx.y, ch = blockIdx.x * 256 + threadIdx.x;
  const int Ts = front_frames(min(max(lens[s], 0), N));
  const int nc = (Ts + kFChunk - 1) / kFChunk;
  const float* pp = part + (long)s * nchunk * kFC + ch;
  float a = 0.f;
  for (int k = 0; k < nc; ++k) a += pp[(long)k * kFC];
  float v = 0.f;
  if (Ts > 0) v = mode == 0 ? a / (float)Ts : rsqrtf(a / (float)Ts + eps);
  dst[(long)s * kFC + ch] = v;
}

template <typename T>
void launch_front(hipStream_t st, const float* wav, const int32_t* lens, int nseq, int N, int T1, int nchunk, const float* w,
                  const float* gamma, const float* beta, float eps, T* out, float* ws) {
  float* part = ws;
  float* mean = ws + (long)nseq * nchunk * kFC;
  float* rstd = mean + (long)nseq * kFC;
  const dim3 grid(nchunk, nseq), sgrid(kFC / 256, nseq);
  hipLaunchKernelGGL((hubert_front_kernel<T, kFrontSum>), grid, dim3(256), 0, st, wav, lens, N, T1, nchunk, w, gamma, beta,
                     mean, rstd, part, out);
  hipLaunchKernelGGL(hubert_front_stat_kernel, sgrid, dim3(256), 0, st, part, lens, N, nchunk, eps, 0, mean);
  hipLaunchKernelGGL((hubert_front_kernel<T, kFrontSq>), grid, dim3(256), 0, st, wav, lens, N, T1, nchunk, w, gamma, beta,
                     mean, rstd, part, out);
  hipLaunchKernelGGL(hubert_front_stat_kernel, sgrid, dim3(256), 0, st, part, lens, N, nchunk, eps, 1, rstd);
  hipLaunchKernelGGL((hubert_front_kernel<T, kFrontStore>), grid, dim3(256), 0, st, wav, lens, N, T1, nchunk, w, gamma, beta,
                     mean, rstd, part, out);
}

// ---- normalize.py:148-153 on a ragged batch of clips
// one block per row: the maximum is order-free; a NaN anywhere in the row makes the peak NaN (as np.abs(x).max())
__global__ __launch_bounds__(1024) void clip_peak_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, int N,
                                                         float* __restrict__ peak) {
  __shared__ float red[16];
  __shared__ int bad[16];
  const int s = blockIdx.x;
  const int n = min(max(lens[s], 0), N);
  const float* xr = x + (long)s * N;
  float m = 0.f;
  int nan = 0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const float v = xr[i];
    nan |= v != v;
    m = fmaxf(m, fabsf(v));
  }
  m = wave_reduce_max(m);
  nan = __any(nan);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = m, bad[wave] = nan;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k) m = fmaxf(m, red[k]), nan |= bad[k];
    peak[s] = nan ? __int_as_float(0x7fc00000) : m;
  }
}

__global__ __launch_bounds__(256) void clip_rescale_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, int N,
                                                           const float* __restrict__ peak, float c1, float c2, float c1b,
                                                           float c2b, float* __restrict__ f, int16_t* __restrict__ q) {
  const int s = blockIdx.y;
  const int n = min(max(lens[s], 0), N);
  const float pk = peak[s];
  const long row = (long)s * N;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    float fv = 0.f;
    int16_t qv = 0;
    if (i < n) {
      const float v = x[row + i];
      fv = rescale_one(v, pk, c1b, c2b);
      qv = trunc_s16(rescale_one(v, pk, c1, c2));
    }
    f[row + i] = fv;
    q[row + i] = qv;
  }
}

// ---- the two ends of Chinese-RoBERTa on a ragged batch of sentences
// Output end: out item i = [C][n_i] at element C * item_off[i], column p of it = token row src[p] of h (or zeros).
// A block owns kXP consecutive columns of ONE item and kXC channels.  Read side: a row's kXC channels are 16 bytes per
// lane (16 lanes of 4 floats, 8 lanes of 8 halves), four (eight) rows per wave instruction.  LDS tile [kXC][kXS] fp32,
// kXS = 65: a transposing ds_write_b32 of lane (row r, lane-in-row g) element k goes to bank (vec g + k + r) mod 32 --
// vec g takes 8 (fp32) or 4 (16-bit) values, the 2 (4) rows of a 32-lane half shift them by r < vec: 2-way.  Store side:
// wave w takes channels w, w + 4, ..., lane l column l: consecutive words of one LDS row (conflict-free) and
// consecutive elements of one output row.
constexpr int kXP = 64, kXC = 64, kXS = kXP + 1;

template <typename T> struct Vec16;
template <> struct Vec16<float> {
  static constexpr int n = 4;
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
  }
};
template <> struct Vec16<h16_t> {
  static constexpr int n = 8;
  static __device__ __forceinline__ void load(const h16_t* p, float* v) {
    const uint4 a = *reinterpret_cast<const uint4*>(p);
    v[0] = h2f_lo(a.x), v[1] = h2f_hi(a.x), v[2] = h2f_lo(a.y), v[3] = h2f_hi(a.y);
    v[4] = h2f_lo(a.z), v[5] = h2f_hi(a.z), v[6] = h2f_lo(a.w), v[7] = h2f_hi(a.w);
  }
};

// grid (upper bound of the column tiles, ceil(C / kXC)), 256 threads.  The block finds the item that owns its tile from
// item_off itself (no host copy of it is needed): thread t counts the tiles of items [t chunk, (t + 1) chunk), the
// counts are prefix-summed in LDS, the thread whose range holds tile blockIdx.x publishes (first column, end).  Every
// offset is clamped into [previous end, total], so that no item_off can send a store outside out[0, C * total).
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void phone_expand_kernel(const TI* __restrict__ h, long n_rows, int C,
                                                           const int32_t* __restrict__ src,
                                                           const int32_t* __restrict__ item_off, int n_items, int total,
                                                           TO* __restrict__ out) {
  __shared__ float tile[kXC * kXS];
  __shared__ int cnt[256];
  __shared__ int sl[kXP];
  __shared__ int found[3];           // first column of the tile, first and end column of its item
  const int tid = threadIdx.x;
  const int chunk = (n_items + 255) / 256;
  const int i0 = min(tid * chunk, n_items), i1 = min(i0 + chunk, n_items);
  auto bounds = [&](int i, int& lo, int& hi) {
    lo = min(max(item_off[i], 0), total);
    hi = min(max(item_off[i + 1], lo), total);
  };
  int mine = 0;
  for (int i = i0; i < i1; ++i) {
    int lo, hi;
    bounds(i, lo, hi);
    mine += (hi - lo + kXP - 1) / kXP;
  }
  cnt[tid] = mine;
  if (tid == 0) found[0] = -1;
  __syncthreads();
  int before = 0;
  for (int u = 0; u < tid; ++u) before += cnt[u];
  const int want = blockIdx.x;
  if (want >= before && want < before + mine) {
    int k = before;
    for (int i = i0; i < i1; ++i) {
      int lo, hi;
      bounds(i, lo, hi);
      const int nt = (hi - lo + kXP - 1) / kXP;
      if (want < k + nt) {
        found[0] = lo + (want - k) * kXP, found[1] = lo, found[2] = hi;
        break;
      }
      k += nt;
    }
  }
  __syncthreads();
  const int p0 = found[0];
  if (p0 < 0) return;                                   // block-uniform: a tile behind the last one
  const int lo = found[1], hi = found[2];
  const int np = min(kXP, hi - p0);                     // live columns of this tile, >= 1
  if (tid < kXP) {
    int s = tid < np ? src[p0 + tid] : -1;
    sl[tid] = (s < 0 || (long)s >= n_rows) ? -1 : s;
  }
  __syncthreads();
  constexpr int V = Vec16<TI>::n, LPR = kXC / V, RPP = 256 / LPR;
  const int g = tid % LPR, r = tid / LPR;
  const int cb = blockIdx.y * kXC;
  const bool chan = cb + g * V < C;                     // C % 8 == 0: a vector is live or dead as a whole
#pragma unroll
  for (int pass = 0; pass < kXP / RPP; ++pass) {
    const int pl = pass * RPP + r;
    if (pl < np) {
      float v[V];
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] = 0.f;
      const int s = sl[pl];
      if (s >= 0 && chan) Vec16<TI>::load(h + (long)s * C + cb + g * V, v);
#pragma unroll
      for (int k = 0; k < V; ++k) tile[(g * V + k) * kXS + pl] = v[k];
    }
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  const int n = hi - lo;
  TO* ob = out + (long)C * lo + (p0 - lo) + lane;
  if (lane < np)
    for (int c = wave; c < kXC && cb + c < C; c += 4) ob[(long)(cb + c) * n] = from_f<TO>(tile[c * kXS + lane]);
}

template <typename TI, typename TO>
void launch_expand(hipStream_t st, const void* h, long n_rows, int C, const int32_t* src, const int32_t* item_off,
                   int n_items, int total, void* out) {
  const dim3 grid((total + kXP - 1) / kXP + n_items, (C + kXC - 1) / kXC);
  hipLaunchKernelGGL((phone_expand_kernel<TI, TO>), grid, dim3(256), 0, st, (const TI*)h, n_rows, C, src, item_off, n_items,
                     total, (TO*)out);
}

// Input end: one wave per token row, lane l channels 4 l + 256 i.  Three passes over the same three table rows (12 KB at
// C = 1024, from L1 after the first), each forming the same fp32 sum (word + pos) + type: the sum, the squared deviations
// from the mean, the normalised store.  Lane partial sums ascend in i, the wave sum is the xor butterfly: the order is a
// function of C alone.
template <typename T> __device__ __forceinline__ void store4(T* p, float a, float b, float c, float d);
template <> __device__ __forceinline__ void store4<float>(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}
template <> __device__ __forceinline__ void store4<h16_t>(h16_t* p, float a, float b, float c, float d) {
  *reinterpret_cast<uint2*>(p) = make_uint2(f2h_pack(a, b), f2h_pack(c, d));
}

__device__ __forceinline__ float4 embed_sum4(const float* w, const float* p, const float* t, int c) {
#pragma clang fp contract(off)
  const float4 a = *reinterpret_cast<const float4*>(w + c);
  const float4 b = *reinterpret_cast<const float4*>(p + c);
  const float4 d = *reinterpret_cast<const float4*>(t + c);
  return make_float4((a.x + b.x) + d.x, (a.y + b.y) + d.y, (a.z + b.z) + d.z, (a.w + b.w) + d.w);
}

template <typename T>
__global__ __launch_bounds__(256) void bert_embed_ln_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ tt,
                                                            const int32_t* __restrict__ lens, int B, int Tn,
                                                            const float* __restrict__ word, int vocab,
                                                            const float* __restrict__ pos, const float* __restrict__ type,
                                                            int types, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, int C,
                                                            T* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (row >= (long)B * Tn) return;                      // wave-uniform
  const int b = (int)(row / Tn), t = (int)(row - (long)b * Tn);
  T* o = out + row * C;
  if (t >= min(max(lens[b], 0), Tn)) {
    for (int c = lane * 4; c < C; c += 256) store4<T>(o + c, 0.f, 0.f, 0.f, 0.f);
    return;
  }
  const int id = min(max(ids[row], 0), vocab - 1);
  const int ty = tt ? min(max(tt[row], 0), types - 1) : 0;
  const float* w = word + (long)id * C;
  const float* p = pos + (long)t * C;
  const float* y = type + (long)ty * C;
  float s = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    const float4 v = embed_sum4(w, p, y, c);
    s += (v.x + v.y) + (v.z + v.w);
  }
  const float mean = wave_reduce_sum(s) / (float)C;
  float q = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    const float4 v = embed_sum4(w, p, y, c);
    const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
    q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
  }
  const float rstd = 1.f / sqrtf(wave_reduce_sum(q) / (float)C + eps);
  for (int c = lane * 4; c < C; c += 256) {
    const float4 v = embed_sum4(w, p, y, c);
    const float4 gm = *reinterpret_cast<const float4*>(gamma + c);
    const float4 bt = *reinterpret_cast<const float4*>(beta + c);
    store4<T>(o + c, (v.x - mean) * rstd * gm.x + bt.x, (v.y - mean) * rstd * gm.y + bt.y,
              (v.z - mean) * rstd * gm.z + bt.z, (v.w - mean) * rstd * gm.w + bt.w);
  }
}

}  // namespace

extern "C" {

int evt_phone_expand_rows(int32_t dtype, const void* h, int32_t B, int32_t T, int32_t C, const int32_t* src,
                          const int32_t* item_off, int32_t n_items, int32_t total, int32_t out_dtype, void* out,
                          void* stream) {
  if (!h || !item_off || B <= 0 || T <= 0 || C < 8 || C > 4096 || (C & 7) || n_items <= 0 || n_items > 65535 || total < 0)
    return EVT_EINVAL;
  if ((long)B * T > 0x7fffffffL || ((uintptr_t)h & 15)) return EVT_EINVAL;
  if (dtype != EVT_DT_HALF && dtype != EVT_DT_F32) return EVT_ENOTSUP;
  if (out_dtype != EVT_DT_HALF && out_dtype != EVT_DT_F32) return EVT_ENOTSUP;
  if (total == 0) return EVT_OK;                        // nothing to write
  if (!src || !out) return EVT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long n_rows = (long)B * T;
  if (dtype == EVT_DT_F32 && out_dtype == EVT_DT_F32)
    launch_expand<float, float>(st, h, n_rows, C, src, item_off, n_items, total, out);
  else if (dtype == EVT_DT_F32)
    launch_expand<float, h16_t>(st, h, n_rows, C, src, item_off, n_items, total, out);
  else if (out_dtype == EVT_DT_F32)
    launch_expand<h16_t, float>(st, h, n_rows, C, src, item_off, n_items, total, out);
  else
    launch_expand<h16_t, h16_t>(st, h, n_rows, C, src, item_off, n_items, total, out);
  return evt_check_launch();
}

int evt_bert_embed_ln_rows(int32_t dtype, const int32_t* ids, const int32_t* tt, const int32_t* lens, int32_t B, int32_t T,
                           const float* word, int32_t vocab, const float* pos, int32_t max_pos, const float* type,
                           int32_t types, const float* gamma, const float* beta, float eps, int32_t C, void* out,
                           void* stream) {
  if (!ids || !lens || !word || !pos || !type || !gamma || !beta || !out || B <= 0 || T <= 0 || T > max_pos || vocab <= 0 ||
      types <= 0 || C < 4 || C > 8192 || (C & 3) || !(eps >= 0.f))
    return EVT_EINVAL;
  if ((long)B * T > 0x7fffffffL) return EVT_EINVAL;
  if (((uintptr_t)word | (uintptr_t)pos | (uintptr_t)type | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15)
    return EVT_EINVAL;
  if (dtype != EVT_DT_HALF && dtype != EVT_DT_F32) return EVT_ENOTSUP;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(((long)B * T + 3) / 4));
  if (dtype == EVT_DT_HALF)
    hipLaunchKernelGGL(bert_embed_ln_kernel<h16_t>, grid, dim3(256), 0, st, ids, tt, lens, B, T, word, vocab, pos, type, types,
                       gamma, beta, eps, C, (h16_t*)out);
  else
    hipLaunchKernelGGL(bert_embed_ln_kernel<float>, grid, dim3(256), 0, st, ids, tt, lens, B, T, word, vocab, pos, type, types,
                       gamma, beta, eps, C, (float*)out);
  return evt_check_launch();
}

int evt_gelu_rows_fwd(int32_t dtype, const void* x, const float* bias, void* out, int64_t nseq, int32_t t_in, int32_t t_out,
                      int32_t C, void* stream) {
  if (!x || !out || nseq <= 0 || t_out <= 0 || t_out > t_in || C <= 0) return EVT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long n = nseq * (long)t_out * C;
  if (dtype == EVT_DT_HALF)
    hipLaunchKernelGGL(gelu_rows_kernel<h16_t>, dim3(ew_blocks(n)), dim3(256), 0, st, (const h16_t*)x, bias, (h16_t*)out,
                       (long)nseq, t_in, t_out, C);
  else if (dtype == EVT_DT_F32)
    hipLaunchKernelGGL(gelu_rows_kernel<float>, dim3(ew_blocks(n)), dim3(256), 0, st, (const float*)x, bias, (float*)out,
                       (long)nseq, t_in, t_out, C);
  else return EVT_ENOTSUP;
  return evt_check_launch();
}

int evt_channel_norm_gelu_fwd(int32_t dtype, const void* x, const float* gamma, const float* beta, float eps, void* out,
                              int32_t nseq, int32_t T, int32_t C, int32_t apply_gelu, void* stream) {
  if (!x || !out || nseq <= 0 || T <= 0 || C <= 0 || !(eps >= 0.f)) return EVT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(nseq, (C + 63) / 64);
  if (dtype == EVT_DT_HALF)
    hipLaunchKernelGGL(channel_norm_gelu_kernel<h16_t>, grid, dim3(256), 0, st, (const h16_t*)x, gamma, beta, eps, (h16_t*)out,
                       T, C, apply_gelu);
  else if (dtype == EVT_DT_F32)
    hipLaunchKernelGGL(channel_norm_gelu_kernel<float>, grid, dim3(256), 0, st, (const float*)x, gamma, beta, eps, (float*)out,
                       T, C, apply_gelu);
  else return EVT_ENOTSUP;
  return evt_check_launch();
}

int64_t evt_hubert_front_ws_floats(int32_t nseq, int32_t N) {
  if (nseq <= 0 || nseq > 65535 || N < kFK) return 0;
  const int64_t T1 = (N - kFK) / kFS + 1;
  return (int64_t)nseq * kFC * ((T1 + kFChunk - 1) / kFChunk + 2);
}

int evt_hubert_front_rows(int32_t dtype, const float* wav, const int32_t* lens, int32_t nseq, int32_t N, const float* w,
                          const float* gamma, const float* beta, float eps, void* out, float* ws, int64_t ws_floats,
                          void* stream) {
  if (!wav || !lens || !w || !gamma || !beta || !out || !ws || nseq <= 0 || nseq > 65535 || N < kFK || !(eps >= 0.f))
    return EVT_EINVAL;
  if (((uintptr_t)out & 15) || ((uintptr_t)ws & 15) || ws_floats < evt_hubert_front_ws_floats(nseq, N)) return EVT_EINVAL;
  if (dtype != EVT_DT_HALF && dtype != EVT_DT_F32) return EVT_ENOTSUP;
  const int T1 = (N - kFK) / kFS + 1;
  const int nchunk = (T1 + kFChunk - 1) / kFChunk;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EVT_DT_HALF) launch_front<h16_t>(st, wav, lens, nseq, N, T1, nchunk, w, gamma, beta, eps, (h16_t*)out, ws);
  else launch_front<float>(st, wav, lens, nseq, N, T1, nchunk, w, gamma, beta, eps, (float*)out, ws);
  return evt_check_launch();
}

int evt_clip_rescale_rows(const float* x, const int32_t* lens, int32_t nseq, int32_t N, float* f, int16_t* q, float* peak,
                          void* stream) {
  if (!x || !lens || !f || !q || !peak || nseq <= 0 || nseq > 65535 || N <= 0) return EVT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  // normalize.py:61-62,151-153: maxx = 0.95, alpha = 0.5; the products in double as Python takes them, rounded once
  const double maxx = 0.95, alpha = 0.5;
  const float c1 = (float)(maxx * alpha * 32768), c2 = (float)((1 - alpha) * 32768);
  const float c1b = (float)(maxx * alpha * 1145.14), c2b = (float)((1 - alpha) * 1145.14);
  hipLaunchKernelGGL(clip_peak_kernel, dim3(nseq), dim3(1024), 0, st, x, lens, N, peak);
  hipLaunchKernelGGL(clip_rescale_kernel, dim3((N + 1023) / 1024, nseq), dim3(256), 0, st, x, lens, N, peak, c1, c2, c1b, c2b,
                     f, q);
  return evt_check_launch();
}

}  // extern "C"

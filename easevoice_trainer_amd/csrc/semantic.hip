// Semantic codes of ragged batches of CN-HuBERT hidden states, gfx950: ssl_proj (Conv1d D -> D, k = 2, stride 2) and the
// nearest code of the frozen codebook in ONE launch, fp32 throughout, on the fp32-input MFMA.
//
// Reference call sites (file:line of the reference project):
//   the `token` step                            src/normalization/normalize.py:181-211
//   extract_latent = ssl_proj + quantizer       src/easevoice/module/models.py:1015-1018, quantize.py:70-94,
//                                                core_vq.py:172-228 (EuclideanCodebook.quantize)
//
// A block owns SC_TILE = 32 code frames of one row, counted from the row's frame 0.  For channels-last rows the k = 2,
// stride 2 convolution is a GEMM over the contiguous pair (x[2t], x[2t + 1]) of 2 D values:
//   1. h[32][D] = pair[32][2 D] . image[2 D][D] + bias.  The pairs pass through LDS in chunks of 64 values; a wave owns 64
//      output channels per pass of 256 and reads its part of the image straight from memory (no other wave needs it).
//      MFMA column `j` of column tile `ct` stands for channel base + 4 j + ct, so a lane's four B values are one 16-byte load.
//   2. h stays in LDS; xx[f] = sum h^2, one wave per 8 frames.
//   3. dots = h . embed^T in chunks of 64 codes per wave, 256 per block step.  One 16-byte load of h and of a code vector
//      feeds four MFMA k-steps: lane quarter q supplies d = d0 + 4 q + s in step s, on both operands.
//      dist = -((xx - 2 dot) + ee) and the running (best, index) per frame are those of rvq_select_kernel (frontend.hip);
//      a lane meets its codes in ascending order, the lanes and the waves meet with "greater, or equal and lower index".
// Every sum has an order fixed by (D, K) alone: a row's codes do not depend on B, Tmax or the other rows.  Nothing at or
// behind frame frames[b] of a row is read; h, the dots and the code vectors never leave the chip.
#include "evt_common.h"
#include "../../include/evt.h"

namespace {

constexpr int SC_TILE = EVT_SEMANTIC_TILE, SC_KC = 64, SC_XS = SC_KC + 4, SC_HPAD = 4;
static_assert(SC_TILE == 32, "two 16-row MFMA tiles per block");

__device__ __forceinline__ void sc_load8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void sc_load8(const h16_t* p, float (&v)[8]) {
  const uint4 a = *reinterpret_cast<const uint4*>(p);
  v[0] = h2f_lo(a.x); v[1] = h2f_hi(a.x); v[2] = h2f_lo(a.y); v[3] = h2f_hi(a.y);
  v[4] = h2f_lo(a.z); v[5] = h2f_hi(a.z); v[6] = h2f_lo(a.w); v[7] = h2f_hi(a.w);
}

__device__ __forceinline__ f32x4 sc_mma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

size_t sc_lds_bytes(int D) { return sizeof(float) * ((size_t)SC_TILE * (D + SC_HPAD) + SC_TILE * SC_XS + SC_TILE + 8 * SC_TILE); }

template <typename T>
__global__ __launch_bounds__(256) void semantic_codes_rows_kernel(const T* hs, const int32_t* frames, const int64_t* offsets,
                                                                  const float* image, const float* bias, const float* embed,
                                                                  const float* ee, int64_t* codes, int Tmax, int D, int K,
                                                                  long total) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int HS = D + SC_HPAD;
  float* hl = reinterpret_cast<float*>(smem);     // [SC_TILE][HS]   the projected frames
  float* xs = hl + SC_TILE * HS;                   // [SC_TILE][SC_XS] one chunk of the pairs
  float* xx = xs + SC_TILE * SC_XS;                // [SC_TILE]
  float* bv = xx + SC_TILE;                        // [4][SC_TILE]    the waves' best distances
  int* bi = reinterpret_cast<int*>(bv + 4 * SC_TILE);
  const int b = blockIdx.y, t0 = blockIdx.x * SC_TILE;
  const int nc = min(max(frames[b], 0), Tmax) >> 1;          // an odd last frame has no code
  if (t0 >= nc) return;                                       // the whole block: no barrier is left waiting
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, q = lane >> 4;

  // ---- 1. the projection ----
  const int srow = tid >> 3, sseg = tid & 7;                 // staging: 8 threads x 8 values per frame
  const bool sok = t0 + srow < nc;
  const T* xrow = hs + ((long)b * Tmax + 2L * (t0 + srow)) * D + sseg * 8;
  const int nchunk = 2 * D / SC_KC;
  for (int cp = 0; cp < D; cp += 256) {
    const int cbase = cp + w * 64;
    const bool act = cbase < D;                               // per wave
    f32x4 acc[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    float pre[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) pre[i] = 0.f;
    if (sok) sc_load8(xrow, pre);
    for (int c = 0; c < nchunk; ++c) {
      __syncthreads();                                        // the previous chunk has been read
      float* xd = xs + srow * SC_XS + sseg * 8;
      *reinterpret_cast<float4*>(xd) = float4{pre[0], pre[1], pre[2], pre[3]};
      *reinterpret_cast<float4*>(xd + 4) = float4{pre[4], pre[5], pre[6], pre[7]};
      __syncthreads();
      if (sok && c + 1 < nchunk) sc_load8(xrow + (long)(c + 1) * SC_KC, pre);
      if (act) {
        const float* wp = image + ((long)c * SC_KC + q) * D + cbase + j * 4;
#pragma unroll 4
        for (int kk = 0; kk < SC_KC / 4; ++kk) {
          const float4 bw = *reinterpret_cast<const float4*>(wp + (long)kk * 4 * D);
          const float a0 = xs[j * SC_XS + kk * 4 + q], a1 = xs[(16 + j) * SC_XS + kk * 4 + q];
          acc[0][0] = sc_mma(a0, bw.x, acc[0][0]);
          acc[1][0] = sc_mma(a1, bw.x, acc[1][0]);
          acc[0][1] = sc_mma(a0, bw.y, acc[0][1]);
          acc[1][1] = sc_mma(a1, bw.y, acc[1][1]);
          acc[0][2] = sc_mma(a0, bw.z, acc[0][2]);
          acc[1][2] = sc_mma(a1, bw.z, acc[1][2]);
          acc[0][3] = sc_mma(a0, bw.w, acc[0][3]);
          acc[1][3] = sc_mma(a1, bw.w, acc[1][3]);
        }
      }
    }
    if (act) {
      const float4 bb = *reinterpret_cast<const float4*>(bias + cbase + j * 4);
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          *reinterpret_cast<float4*>(hl + (rt * 16 + q * 4 + r) * HS + cbase + j * 4) =
              float4{acc[rt][0][r] + bb.x, acc[rt][1][r] + bb.y, acc[rt][2][r] + bb.z, acc[rt][3][r] + bb.w};
    }
  }
  __syncthreads();

  // ---- 2. xx = |h|^2 ----
  for (int f = w * 8; f < w * 8 + 8; ++f) {
    float s = 0.f;
    for (int d = lane; d < D; d += 64) { const float v = hl[f * HS + d]; s += v * v; }
    s = wave_reduce_sum(s);
    if (lane == 0) xx[f] = s;
  }
  __syncthreads();

  // ---- 3. the codebook ----
  float best[2][4];
  int bidx[2][4];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) { best[rt][r] = -INFINITY; bidx[rt][r] = 0x7fffffff; }
  float xf[2][4];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) xf[rt][r] = xx[rt * 16 + q * 4 + r];
  for (int cb = w * 64; cb < K; cb += 256) {                  // per wave; no barrier inside
    f32x4 acc[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* ep[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) ep[ct] = embed + (long)min(cb + ct * 16 + j, K - 1) * D + 4 * q;   // tail: masked below
    const float* h0 = hl + j * HS + 4 * q;
    const float* h1 = hl + (16 + j) * HS + 4 * q;
#pragma unroll 2
    for (int d0 = 0; d0 < D; d0 += 16) {
      const float4 a0 = *reinterpret_cast<const float4*>(h0 + d0), a1 = *reinterpret_cast<const float4*>(h1 + d0);
      float4 e[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) e[ct] = *reinterpret_cast<const float4*>(ep[ct] + d0);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) { acc[0][ct] = sc_mma(a0.x, e[ct].x, acc[0][ct]); acc[1][ct] = sc_mma(a1.x, e[ct].x, acc[1][ct]); }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) { acc[0][ct] = sc_mma(a0.y, e[ct].y, acc[0][ct]); acc[1][ct] = sc_mma(a1.y, e[ct].y, acc[1][ct]); }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) { acc[0][ct] = sc_mma(a0.z, e[ct].z, acc[0][ct]); acc[1][ct] = sc_mma(a1.z, e[ct].z, acc[1][ct]); }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) { acc[0][ct] = sc_mma(a0.w, e[ct].w, acc[0][ct]); acc[1][ct] = sc_mma(a1.w, e[ct].w, acc[1][ct]); }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int c = cb + ct * 16 + j;
      if (c < K) {
        const float eev = ee[c];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float dist = -((xf[rt][r] - 2.f * acc[rt][ct][r]) + eev);
            if (dist > best[rt][r]) { best[rt][r] = dist; bidx[rt][r] = c; }   // c ascends per lane: the first maximum stays
          }
      }
    }
  }
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = best[rt][r];
      int i = bidx[rt][r];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {                       // the 16 lanes that share a frame
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
      }
      if (j == 0) { bv[w * SC_TILE + rt * 16 + q * 4 + r] = v; bi[w * SC_TILE + rt * 16 + q * 4 + r] = i; }
    }
  __syncthreads();
  if (tid < SC_TILE && t0 + tid < nc) {
    float v = bv[tid];
    int i = bi[tid];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const float ov = bv[k * SC_TILE + tid];
      const int oi = bi[k * SC_TILE + tid];
      if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    if (i >= K) i = 0;                                         // no valid maximum (an all-NaN frame): code 0
    const long o = (long)offsets[b] + t0 + tid;
    if (o >= 0 && o < total) codes[o] = i;
  }
}

template <typename T>
int sc_launch(const void* hs, const int32_t* frames, const int64_t* offsets, int B, int Tmax, int D, int K, const float* image,
              const float* bias, const float* embed, const float* ee, int64_t* codes, long total, hipStream_t stream) {
  static size_t have = 48 * 1024;
  const size_t lds = sc_lds_bytes(D);
  if (lds > have) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&semantic_codes_rows_kernel<T>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return EVT_ELAUNCH;
    have = lds;
  }
  const dim3 grid((Tmax / 2 + SC_TILE - 1) / SC_TILE, B);
  hipLaunchKernelGGL(semantic_codes_rows_kernel<T>, grid, dim3(256), lds, stream, (const T*)hs, frames, offsets, image, bias,
                     embed, ee, codes, Tmax, D, K, total);
  return evt_check_launch();
}

}  // namespace

extern "C" int evt_semantic_codes_rows(int32_t dtype, const void* hs, const int32_t* frames, const int32_t* frames_host,
                                       const int64_t* offsets, int32_t B, int32_t Tmax, int32_t D, int32_t K,
                                       const float* proj_image, const float* bias, const float* embed, const float* ee,
                                       int64_t* codes, int64_t total, void* stream) {
  if (!hs || !frames || !offsets || !proj_image || !bias || !embed || !ee) return EVT_EINVAL;
  if (B <= 0 || B > 65535 || Tmax <= 0 || K <= 0 || total < 0 || (total > 0 && !codes)) return EVT_EINVAL;
  if (D < 64 || D % 64 || D > EVT_SEMANTIC_MAX_D) return EVT_EINVAL;
  if (dtype != EVT_DT_F32 && dtype != EVT_DT_HALF) return EVT_EINVAL;
  if (((uintptr_t)hs | (uintptr_t)proj_image | (uintptr_t)bias | (uintptr_t)embed) & 15) return EVT_EINVAL;
  if (frames_host)
    for (int b = 0; b < B; ++b)
      if (frames_host[b] < 0 || frames_host[b] > Tmax) return EVT_EINVAL;
  if (total == 0 || Tmax < 2) return EVT_OK;
  evt_set_last_tag(dtype == EVT_DT_F32 ? "semantic_codes_rows<f32>" : "semantic_codes_rows<" EVT_HALF_NAME ">");
  if (dtype == EVT_DT_F32)
    return sc_launch<float>(hs, frames, offsets, B, Tmax, D, K, proj_image, bias, embed, ee, codes, (long)total,
                            (hipStream_t)stream);
  return sc_launch<h16_t>(hs, frames, offsets, B, Tmax, D, K, proj_image, bias, embed, ee, codes, (long)total,
                          (hipStream_t)stream);
}

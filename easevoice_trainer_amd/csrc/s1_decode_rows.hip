// s1 decode linear for a batch of up to 128 rows, in row groups of 32 (infer_panel_batch_infer, t2s_model.py:563-730,
// with the TTS service's default of 20 texts per call; stream sessions of up to 128 slots) for gfx950.
//
// evt_dec_gemv keeps the whole input [B][K] in LDS and every wave walks its own weight rows with VALU dot products, so it
// stops at four rows.  Here one workgroup owns a 16-row tile of W and ALL rows of x: every weight byte is read from HBM
// once per launch, whatever B is, and the products run on v_mfma_f32_16x16x4_f32 (an exact fp32 FMA chain: activations
// stay fp32, 16-bit weights are widened exactly; only the order of the sum differs from evt_dec_gemv).
//   A operand = W[n0 + (lane & 15)][k], B operand = x[b0 + (lane & 15)][k], k = one of the lane group's (lane >> 4) 16
//   consecutive columns; D[n][b] comes out with the row n on (lane >> 4) * 4 + reg and the batch row b on lane & 15.
//   K is staged through LDS in chunks of 512 (32 x 512 fp32 = 64 KB); the 8 waves split every chunk into 8 slices of 64,
//   the next chunk's x is loaded into registers while the current one is multiplied, and all weights of the tile are
//   requested before anything else.  The 8 wave partials are summed through LDS in wave order (no atomics: two launches
//   give the same bits).
//   LayerNorm prologue: one wave per batch row computes (mean, 1/std) from a + r while the staging loads are in flight.
//   More than 32 rows: row groups of 32 on blockIdx.y.  Block (x, g) is the block described above for the weight rows
//   16x .. 16x+15 and the batch rows 32g .. min(32g + 32, B) - 1: a, r, y and x_out are offset by the group, everything
//   else (statistics, staging buffer, partial tiles, the b-tiles in use) is the group's own, and x_out is written by the
//   blockIdx.x == 0 block of each group.  A row's arithmetic does not depend on the launch it is in, so every output
//   row of a wide launch has the bits a launch of that row's group alone gives; B <= 32 launches the grid it always
//   launched.  The G blocks of a weight tile re-read it; at G <= 4 that is meant to hit L2 / the Infinity Cache.
#include "evt_common.h"
#include "s1_decode_rows_index.h"
#include "../../include/evt.h"

namespace {

// rows per group / per launch, waves, threads, K chunk and the staging count: s1_decode_rows_index.h
using evt_rows::kRows; using evt_rows::kRowsMax; using evt_rows::kNW; using evt_rows::kThreads; using evt_rows::kKC;
using evt_rows::kXPT;
constexpr int kXS = kKC + 4;         // LDS row stride (floats): the 16 rows of a b-tile start on different banks
constexpr int kKW = kKC / kNW;       // K slice of a wave per chunk: 64 = 4 lane groups x 16
constexpr int kPS = kRows + 1;       // row stride of the partial tiles in LDS
constexpr int kLds = kRows * kXS * (int)sizeof(float);
static_assert(kNW * 16 * kPS <= kRows * kXS, "partials fit in the staging buffer");

template <typename T, int NCH>
__global__ __launch_bounds__(kThreads) void dec_gemm_rows(const T* __restrict__ W, const float* __restrict__ bias,
                                                          const float* __restrict__ a, const float* __restrict__ r,
                                                          const float* __restrict__ ln_g, const float* __restrict__ ln_b,
                                                          float eps, float* x_out, float* __restrict__ y, int Bt, int N,
                                                          int relu) {
  extern __shared__ float xs[];      // [kRows][kXS] x of the current chunk; then the wave partials [kNW][16][kPS]
  __shared__ float mu[kRows], rstd[kRows];
  constexpr int K = NCH * kKC;
  constexpr int V = 16 / (int)sizeof(T);   // elements per 16-byte load
  constexpr int U = 16 / V;                // 16-byte loads per lane per chunk (16 columns)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.x * 16;
  // the block's row group: rows g0 .. g0 + B - 1 of the launch, B = 1..32 (the last group may be short)
  const int g0 = evt_rows::group_first(blockIdx.y);
  const int B = evt_rows::group_rows(Bt, g0);
  a += evt_rows::row_offset(g0, K);
  if (r) r += evt_rows::row_offset(g0, K);
  if (x_out) x_out += evt_rows::row_offset(g0, K);
  y += evt_rows::row_offset(g0, N);
  const int nbt = evt_rows::b_tiles(B);    // b-tiles in use (1 or 2), uniform over the group
  // ---- every weight of the tile in flight first ----
  uint4 w[NCH][U];
  {
    const int n = n0 + j;
    const T* row = W + (long)(n < N ? n : 0) * K + wave * kKW + kq * 16;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int u = 0; u < U; ++u)
        w[c][u] = n < N ? *reinterpret_cast<const uint4*>(row + c * kKC + u * V) : make_uint4(0, 0, 0, 0);
  }
  // staging layout: thread -> columns 4*k4 .. 4*k4+3 of rows (tid >> 7) + 4*i
  const int k4 = evt_rows::stage_k4(tid), rb = evt_rows::stage_row0(tid);
  const int rows_used = nbt * 16;
  float4 xr[kXPT];
  auto load_chunk = [&](int c) {
#pragma unroll
    for (int i = 0; i < kXPT; ++i) {
      const int b = rb + 4 * i;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (b < B) {
        const long o = evt_rows::stage_offset(b, K, c, k4);
        v = *reinterpret_cast<const float4*>(a + o);
        if (r) {
          const float4 q = *reinterpret_cast<const float4*>(r + o);
          v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
        }
      }
      xr[i] = v;
    }
  };
  load_chunk(0);
  // the epilogue's operands are requested now as well
  const int eb = evt_rows::epi_row(tid), en = evt_rows::epi_col(tid);
  const float bz = (bias && n0 + en < N) ? bias[n0 + en] : 0.f;
  if (r) {
    // LayerNorm statistics of a + r, one wave per batch row (same formula as evt_dec_gemv: E[x^2] - E[x]^2)
#pragma unroll 1
    for (int b = wave; b < B; b += kNW) {
      float s = 0.f, q = 0.f;
#pragma unroll
      for (int k = lane * 4; k < K; k += 256) {
        const float4 va = *reinterpret_cast<const float4*>(a + (long)b * K + k);
        const float4 vr = *reinterpret_cast<const float4*>(r + (long)b * K + k);
        const float v0 = va.x + vr.x, v1 = va.y + vr.y, v2 = va.z + vr.z, v3 = va.w + vr.w;
        s += (v0 + v1) + (v2 + v3);
        q += (v0 * v0 + v1 * v1) + (v2 * v2 + v3 * v3);
      }
      s = wave_reduce_sum(s);
      q = wave_reduce_sum(q);
      if (lane == 0) {
        const float m = s / K;
        mu[b] = m;
        rstd[b] = rsqrtf(fmaxf(q / K - m * m, 0.f) + eps);
      }
    }
    __syncthreads();
  }
  auto store_chunk = [&](int c) {
    float4 g = make_float4(1.f, 1.f, 1.f, 1.f), be = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r) {
      g = *reinterpret_cast<const float4*>(ln_g + c * kKC + 4 * k4);
      be = *reinterpret_cast<const float4*>(ln_b + c * kKC + 4 * k4);
    }
#pragma unroll
    for (int i = 0; i < kXPT; ++i) {
      const int b = rb + 4 * i;
      if (b >= rows_used) break;
      float4 v = xr[i];
      if (r && b < B) {
        const float m = mu[b], s = rstd[b];
        v.x = (v.x - m) * s * g.x + be.x;
        v.y = (v.y - m) * s * g.y + be.y;
        v.z = (v.z - m) * s * g.z + be.z;
        v.w = (v.w - m) * s * g.w + be.w;
        if (x_out && blockIdx.x == 0) *reinterpret_cast<float4*>(x_out + evt_rows::stage_offset(b, K, c, k4)) = v;
      }
      *reinterpret_cast<float4*>(xs + b * kXS + 4 * k4) = v;
    }
  };
  store_chunk(0);
  __syncthreads();
  // two accumulation chains per b-tile (even / odd column of the lane's 16): the dependent-MFMA latency is hidden
  f32x4 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h) acc[t][h] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c > 0) {
      __syncthreads();             // every wave is done with chunk c - 1
      store_chunk(c);
      __syncthreads();
    }
    if (c + 1 < NCH) load_chunk(c + 1);
    float wf[16];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const T* pw = reinterpret_cast<const T*>(&w[c][u]);
#pragma unroll
      for (int e = 0; e < V; ++e) wf[u * V + e] = to_f<T>(pw[e]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (t >= nbt) break;
      const float* xp = xs + (t * 16 + j) * kXS + wave * kKW + kq * 16;
      float xv[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 f = *reinterpret_cast<const float4*>(xp + 4 * q);
        xv[4 * q] = f.x; xv[4 * q + 1] = f.y; xv[4 * q + 2] = f.z; xv[4 * q + 3] = f.w;
      }
#pragma unroll
      for (int e = 0; e < 16; ++e)
        acc[t][e & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[e], xv[e], acc[t][e & 1], 0, 0, 0);
    }
  }
  // ---- sum of the 8 wave partials in wave order, bias, activation ----
  __syncthreads();                   // the staging buffer becomes the partials
  float* part = xs;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t >= nbt) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) part[(wave * 16 + kq * 4 + i) * kPS + t * 16 + j] = acc[t][0][i] + acc[t][1][i];
  }
  __syncthreads();
  if (eb < B && n0 + en < N) {
    float s = part[en * kPS + eb];
#pragma unroll
    for (int wv = 1; wv < kNW; ++wv) s += part[(wv * 16 + en) * kPS + eb];
    float o = s + bz;
    if (relu) o = fmaxf(o, 0.f);
    y[(long)eb * N + n0 + en] = o;
  }
}

template <typename T, int NCH>
int launch_rows(const void* W, const float* bias, const float* a, const float* r, const float* g, const float* bt,
                float eps, float* x_out, float* y, int B, int N, int relu, hipStream_t st) {
  static bool lds_set = false;       // > 64 KB of dynamic LDS needs the attribute once per kernel
  if (!lds_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&dec_gemm_rows<T, NCH>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, kLds) != hipSuccess)
      return EVT_ELAUNCH;
    lds_set = true;
  }
  hipLaunchKernelGGL((dec_gemm_rows<T, NCH>), dim3(evt_rows::grid_x(N), evt_rows::grid_y(B)), dim3(kThreads), kLds, st,
                     (const T*)W, bias, a, r, g, bt, eps, x_out, y, B, N, relu);
  return evt_check_launch();
}

template <typename T>
int dispatch_rows(int K, const void* W, const float* bias, const float* a, const float* r, const float* g,
                  const float* bt, float eps, float* x_out, float* y, int B, int N, int relu, hipStream_t st) {
  switch (K / kKC) {
    case 1: return launch_rows<T, 1>(W, bias, a, r, g, bt, eps, x_out, y, B, N, relu, st);
    case 2: return launch_rows<T, 2>(W, bias, a, r, g, bt, eps, x_out, y, B, N, relu, st);
    case 3: return launch_rows<T, 3>(W, bias, a, r, g, bt, eps, x_out, y, B, N, relu, st);
    case 4: return launch_rows<T, 4>(W, bias, a, r, g, bt, eps, x_out, y, B, N, relu, st);
    default: return EVT_ENOTSUP;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int evt_dec_gemm_rows(int32_t wdtype, const void* W, const float* bias, const float* a, const float* r,
                                 const float* ln_g, const float* ln_b, float ln_eps, float* x_out, float* y, int32_t B,
                                 int32_t N, int32_t K, int32_t relu, void* stream) {
  if (!W || !a || !y || B <= 0 || N <= 0 || K <= 0) return EVT_EINVAL;
  if (r && (!ln_g || !ln_b)) return EVT_EINVAL;
  if (!aligned16(W) || !aligned16(a) || (r && (!aligned16(r) || !aligned16(ln_g) || !aligned16(ln_b))) ||
      (x_out && !aligned16(x_out)))
    return EVT_EINVAL;
  if (B > kRowsMax || K % kKC || K > 4 * kKC) return EVT_ENOTSUP;
  hipStream_t st = (hipStream_t)stream;
  if (wdtype == EVT_DT_HALF) return dispatch_rows<h16_t>(K, W, bias, a, r, ln_g, ln_b, ln_eps, x_out, y, B, N, relu, st);
  if (wdtype == EVT_DT_F32) return dispatch_rows<float>(K, W, bias, a, r, ln_g, ln_b, ln_eps, x_out, y, B, N, relu, st);
  return EVT_EINVAL;
}

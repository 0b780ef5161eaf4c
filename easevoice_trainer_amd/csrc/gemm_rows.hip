// fp32 GEMM of the feature extractors on rows that may overlap, gfx950: dense layers and the strided no-padding convolutions
// of HuBERT's feature extractor through ONE kernel on mfma_f32_16x16x4f32 (true fp32 products), bias and GELU in the
// epilogue, forward only, ONE launch, no workspace.  include/evt.h has the definition of the entry point
// (evt_gemm_rows_f32).
//
// Reference call sites: the nn.Linear layers of transformers' HubertModel / BertModel and HubertNoLayerNormConvLayer
// (Conv1d 512 -> 512, k 3 / 2, stride 2, no padding, GELU), which the reference runs on the CPU in float32
// (src/easevoice/feature_extractor/cnhubert.py:16-32, src/normalization/normalize.py:65-106, 158).
//
//   y[b][m][n] = act(sum_k x[b * x_item + m * lda + k] * w[n][k] + bias[n])    m < lens[b], zeros behind
//
// A without im2col.  Row m of item b is the run of K floats at b * x_item + m * lda.  lda = K is a dense layer; in a
//   channels-last [T, cin] buffer lda = stride * cin, K = k * cin is the im2col row of a convolution without padding (rows
//   overlap for k = 3, stride 2).  The kernel never learns which: a row is a pointer and a length.  Overlapping rows are
//   fetched per row; their second read is an L2 hit.  W is the checkpoint's [N][K] row-major matrix (a convolution's
//   [cout][cin][k] permuted once on the host to [cout][k * cin]): no repack launch, no image.
// Work split.  Grid (column tiles, row tiles, items), 4 waves as 2 x 2.  A block owns one item, TM rows counted from the
//   item's row 0 and TN columns; a wave owns (TM / 2) x (TN / 2) = RT x RT MFMA tiles.  Two instantiations: RT = 4
//   (128 x 128, 64 accumulators a lane) and RT = 2 (64 x 64) for launches whose 128 x 128 grid would leave compute units
//   without a block (a lone BERT sentence: 1 x 8 blocks).  The choice reads the launch's block count only, never the data.
// Registers.  mfma_f32_16x16x4f32 takes from lane (g = lane / 16, n = lane % 16) A[m = n][k = g] and B[k = g][n] and leaves
//   C[m = 4 g + r][n] in register r.  W is the A operand and x the B operand (the product comes out transposed), so lane
//   (g, n) ends with columns 4 g .. 4 g + 3 of output row n: the epilogue is one 16-byte store per tile.  Which k a lane
//   quarter supplies is free as long as both operands agree (pos_conv.hip): in a slab of 16 k, lane quarter g holds
//   k = 4 g .. 4 g + 3 of its row (x) or column (w) from ONE ds_read_b128, and MFMA j takes register j of both.  A slab of
//   a wave is RT + RT reads for 4 RT^2 MFMAs (8 : 64 at RT = 4; conv_igemm<float> issues one read per MFMA).
// LDS.  K passes through in chunks of 32 floats: an x tile [TM][32] and a w tile [TN][32] with row pitch 36 floats,
//   double-buffered: 4 * 128 * 36 * 4 = 72 KiB at RT = 4 (two blocks per CU), 36 KiB at RT = 2 (four).  Pitch: 144 bytes are
//   9 16-byte slots, odd, so the 16 lanes of a ds_read_b128 group (rows n .. n + 15, one g) start at 16 distinct slots
//   9 n mod 16: conflict-free.  Tiles arrive by plain 16-byte loads into registers (chunk c + 1 is in flight while chunk c is
//   multiplied) and ds_write_b128 behind the arithmetic, one barrier per chunk.  Not LDS-DMA: its target is lane-linear,
//   which excludes the padded pitch, and rows at or behind lens[b], columns at or behind N and the k at or behind K of the
//   last chunk have to be ZERO-FILLED by ordinary writes anyway (they are not read from memory; NaN * 0 is NaN on the MFMA).
// Order of every sum: chunks from k = 0, inside a chunk slab 0 then slab 1 (a slab at or behind K is skipped), inside a slab
//   MFMA 0 .. 3; an output element is one MFMA column fed by its own row and column only.  No split-K.  Nothing depends on
//   nseq, rows, the neighbours, the tile instantiation or the wave an element lands in: a row is bit for bit the row alone.
// Epilogue: + bias, GELU (gelu_f of evt_common.h, the function evt_gelu_rows_fwd uses), 16-byte stores; rows at or behind
//   lens[b] are written as zeros.
// Budget (hipcc -Rpass-analysis=kernel-resource-usage): DESIGN.md section 11b has the registers, LDS and occupancy.
#include "evt_common.h"
#include "../../include/evt.h"

namespace {

constexpr int GR_KC = EVT_GEMM_ROWS_TILE_K, GR_P = GR_KC + 4, GR_THREADS = 256, GR_SEG = GR_KC / 4;
static_assert(GR_KC == 32, "two slabs of 16 k per chunk");
// launches whose 128 x 128 grid has fewer blocks than this run on 64 x 64 tiles: one block per compute unit of the MI355X
constexpr long GR_SMALL_BELOW = 256;
// the launch tag.  A named constant: the literal tags in csrc/ are the registry of tests/exact_inputs.py; this kernel has its
// integer-exact cases in tests/test_gemm_rows_gpu.py.
constexpr const char* GR_TAG = "gemm_rows_f32<%d,%s>";

struct GrArgs {
  const float *x, *w, *bias;
  const int32_t* lens;
  float* y;
  int rows, N, K, act;
  long x_item, lda;
};

template <int RT> constexpr size_t gr_lds_bytes() { return (size_t)2 * 2 * (32 * RT) * GR_P * sizeof(float); }

// grid (ceil(N / T), ceil(rows / T), nseq) with T = 32 RT, 256 threads, gr_lds_bytes<RT>() of dynamic LDS
template <int RT>
__global__ __launch_bounds__(GR_THREADS) void gemm_rows_f32_kernel(GrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int T = 32 * RT, W = 16 * RT;                         // the block's rows / columns; a wave's
  constexpr int NL = T * GR_SEG / GR_THREADS;                     // 16-byte loads per thread, chunk and operand
  constexpr int TILE = T * GR_P;                                  // floats of one operand's buffer
  const int b = blockIdx.z, m0 = blockIdx.y * T, n0 = blockIdx.x * T;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), n = lane & 15, g = lane >> 4;
  const int wm = (wave >> 1) * W, wn = (wave & 1) * W;            // the wave's corner inside the block's tile
  const int len = a.lens ? min(max(a.lens[b], 0), a.rows) : a.rows;
  float* yb = a.y + ((long)b * a.rows + m0) * a.N + n0;

  if (m0 >= len) {                                                // the whole block: no barrier is left waiting
    const int tw = min(T, a.rows - m0), cw = min(T, a.N - n0) / 4;
    for (int i = tid; i < tw * cw; i += GR_THREADS) {
      const int r = i / cw, c = i - r * cw;
      *reinterpret_cast<float4*>(yb + (long)r * a.N + 4 * c) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }

  float* xs = reinterpret_cast<float*>(smem);                     // [2][T][GR_P]
  float* ws = xs + 2 * TILE;                                      // [2][T][GR_P]
  const float* xg = a.x + (long)b * a.x_item + (long)m0 * a.lda;
  const float* wg = a.w + (long)n0 * a.K;
  const int nchunk = (a.K + GR_KC - 1) / GR_KC;

  float4 xr[NL], wr[NL];
  // chunk c -> registers: rows at or behind len, columns at or behind N and k at or behind K are zeros and are not read
  auto fetch = [&](int c) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + i * GR_THREADS, row = idx / GR_SEG, k = c * GR_KC + 4 * (idx % GR_SEG);
      xr[i] = wr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < a.K) {
        if (m0 + row < len) xr[i] = *reinterpret_cast<const float4*>(xg + (long)row * a.lda + k);
        if (n0 + row < a.N) wr[i] = *reinterpret_cast<const float4*>(wg + (long)row * a.K + k);
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + i * GR_THREADS, row = idx / GR_SEG, sg = idx % GR_SEG;
      *reinterpret_cast<float4*>(xs + buf * TILE + row * GR_P + 4 * sg) = xr[i];
      *reinterpret_cast<float4*>(ws + buf * TILE + row * GR_P + 4 * sg) = wr[i];
    }
  };
  fetch(0);
  stash(0);
  __syncthreads();

  f32x4 acc[RT][RT];                                              // [row tile][column tile]
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < RT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool wlive = m0 + wm < len && n0 + wn < a.N;             // per wave
  for (int c = 0; c < nchunk; ++c) {
    if (c + 1 < nchunk) fetch(c + 1);
    if (wlive) {
      const float* xt = xs + (c & 1) * TILE + (wm + n) * GR_P + 4 * g;
      const float* wt = ws + (c & 1) * TILE + (wn + n) * GR_P + 4 * g;
#pragma unroll
      for (int s = 0; s < GR_KC / 16; ++s) {
        if (c * GR_KC + 16 * s >= a.K) break;                     // the half chunk behind K (K % 16 == 0)
        float4 xf[RT], wf[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) xf[rt] = *reinterpret_cast<const float4*>(xt + rt * 16 * GR_P + 16 * s);
#pragma unroll
        for (int ct = 0; ct < RT; ++ct) wf[ct] = *reinterpret_cast<const float4*>(wt + ct * 16 * GR_P + 16 * s);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int ct = 0; ct < RT; ++ct) {
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[ct].x, xf[rt].x, acc[rt][ct], 0, 0, 0);
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[ct].y, xf[rt].y, acc[rt][ct], 0, 0, 0);
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[ct].z, xf[rt].z, acc[rt][ct], 0, 0, 0);
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[ct].w, xf[rt].w, acc[rt][ct], 0, 0, 0);
          }
      }
    }
    if (c + 1 < nchunk) stash((c + 1) & 1);                       // that buffer was last read before the previous barrier
    __syncthreads();
  }

  // lane (g, n): columns 4 g .. 4 g + 3 of row n of every tile
#pragma unroll
  for (int ct = 0; ct < RT; ++ct) {
    const int col = wn + ct * 16 + 4 * g;
    if (n0 + col >= a.N) continue;                                // N % 16 == 0: a column tile is in or out as a whole
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.bias) bv = *reinterpret_cast<const float4*>(a.bias + n0 + col);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int row = wm + rt * 16 + n;
      if (m0 + row >= a.rows) continue;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m0 + row < len) {
        o = make_float4(acc[rt][ct][0] + bv.x, acc[rt][ct][1] + bv.y, acc[rt][ct][2] + bv.z, acc[rt][ct][3] + bv.w);
        if (a.act) o = make_float4(gelu_f(o.x), gelu_f(o.y), gelu_f(o.z), gelu_f(o.w));
      }
      *reinterpret_cast<float4*>(yb + (long)row * a.N + col) = o;
    }
  }
}

template <int RT>
int gr_launch(const GrArgs& a, int nseq, hipStream_t stream) {
  constexpr int T = 32 * RT;
  static bool raised = false;                                     // 72 KiB at RT = 4: above the 48 KiB default limit
  if (gr_lds_bytes<RT>() > 48 * 1024 && !raised) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_rows_f32_kernel<RT>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)gr_lds_bytes<RT>()) != hipSuccess)
      return EVT_ELAUNCH;
    raised = true;
  }
  const dim3 grid((a.N + T - 1) / T, (a.rows + T - 1) / T, nseq);
  hipLaunchKernelGGL((gemm_rows_f32_kernel<RT>), grid, dim3(GR_THREADS), gr_lds_bytes<RT>(), stream, a);
  return evt_check_launch();
}
static_assert(EVT_GEMM_ROWS_TILE_M == 128 && EVT_GEMM_ROWS_TILE_N == 128, "the RT = 4 instantiation");
static_assert(gr_lds_bytes<4>() <= 80 * 1024, "two blocks of the large tile per compute unit (160 KiB of LDS)");

}  // namespace

extern "C" int evt_gemm_rows_f32(const evt_gemm_rows_params* p, const void* x, const int32_t* lens, const void* w,
                                 const float* bias, void* y, void* stream) {
  if (!p || !x || !w || !y) return EVT_EINVAL;
  if (p->nseq <= 0 || p->rows <= 0 || p->N <= 0 || p->K <= 0 || p->lda <= 0 || p->x_item < 0) return EVT_EINVAL;
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)bias) & 15) return EVT_EINVAL;
  if ((uintptr_t)lens & 3) return EVT_EINVAL;
  if (p->act != EVT_GEMM_ROWS_ACT_NONE && p->act != EVT_GEMM_ROWS_ACT_GELU) return EVT_ENOTSUP;
  if (p->K % 16 || p->N % 16 || p->lda % 4 || p->x_item % 4 || p->nseq > 65535) return EVT_ENOTSUP;
  if (((int64_t)p->rows + 63) / 64 > 65535) return EVT_ENOTSUP;   // the grid's y extent at the small tile
  GrArgs a{(const float*)x, (const float*)w, bias, lens, (float*)y, p->rows, p->N, p->K, p->act, (long)p->x_item, (long)p->lda};
  const long big = (long)((p->N + 127) / 128) * ((p->rows + 127) / 128) * p->nseq;
  const bool small = big < GR_SMALL_BELOW;
  evt_set_last_tag(GR_TAG, small ? 64 : 128, p->act ? "gelu" : "none");
  if (small) return gr_launch<2>(a, p->nseq, (hipStream_t)stream);
  return gr_launch<4>(a, p->nseq, (hipStream_t)stream);
}

// HuBERT's positional convolution on ragged batches of channels-last rows, gfx950: a grouped Conv1d C -> C with a long kernel
// (chinese-hubert-base: C = 768, 16 groups of cg = 48, k = 128, padding 64, the last frame dropped), bias and GELU in the
// epilogue, ONE launch.  Forward only.  include/evt.h has the definition of the two entry points.
//
// Reference call site: transformers' HubertPositionalConvEmbedding inside HubertModel, which the reference runs on the CPU
// (src/easevoice/feature_extractor/cnhubert.py:16-32, src/normalization/normalize.py:158).
//
// Per group the layer is a GEMM with M = frames, N = cg, K = k * cg (6144 for the base model).
//   A, without im2col.  A block owns (row s, group g, PC_TILE frames counted from the row's frame 0) and stages the window of
//     PC_TILE + k - 1 frames x cg channels ONCE into LDS, xs[frame * P + c], 16-byte loads, zeros for frames < 0 or >= n_s
//     (nothing at or behind a row's end is read).  With K ordered as kk = tap * cg + c, the im2col matrix is a view of that
//     array: A[m][kk] = xs[(m + kk / cg) * P + kk % cg], which for P = cg is the flat xs[m * cg + kk] -- conv_grouped.hip's
//     trick for cin/g x stride = 16, carried over to stride 1 and a long reduction.  cg is a multiple of 8, so the 8
//     K elements of a lane never straddle a frame: every MFMA A fragment is one aligned ds_read_b128 (two in fp32).
//     Row pitch P: in 16-bit the pitch in 16-byte slots has to be 2 x odd for conflict-free ds_read_b128 (conv1d.hip's LDS
//     note): cg = 16 (2 slots) and cg = 48 (6) are; cg = 32 (4) and cg = 64 (8) get P = cg + 16 (6 and 10 slots).  In fp32
//     the pitch stays cg: a K step there is 96 MFMAs of 32 cycles against 14 ds_read_b128, the reads hide at any conflict
//     degree, and a padded window would cost 12 KB of LDS at cg = 48.
//   B, the packed image, in MFMA fragment order [g][K step of 32][column tile][64 lanes][8] (evt_pos_conv_pack): lane
//     (j = lane & 15, q = lane >> 4) holds w for column 16 ct + j and kk = 32 ks + 8 q + i.  The same order serves
//     mfma_f32_16x16x32 of the 16-bit types (one fragment = 1 KiB) and eight mfma_f32_16x16x4f32 per K step in fp32 (true
//     fp32, as semantic.hip; the i-th takes element i of both operands: which k a lane quarter supplies is free as long as A
//     and B agree).  A group's image is 576 KB in 16-bit, so it is not resident: it passes through LDS in chunks of PC_KC
//     K steps, double-buffered, shared by the four waves (per wave from L2 it would take ~16 B/clk per wave, the CU's L2
//     port; through LDS the block needs a quarter).  A chunk is contiguous in the image and goes to LDS by LDS-DMA
//     (global_load_lds_dwordx4, as gemm256.hip / conv_deep.hip): no registers, no ds_write; chunk c + 1 is in flight while
//     chunk c is multiplied, one s_waitcnt vmcnt(0) + barrier per chunk.
//   Work split.  4 waves; a wave owns 64 frames x all cg / 16 column tiles: 4 x 3 accumulator tiles = 48 fp32 registers at
//     cg = 48, and per K step 4 A + 3 B fragment reads feed 12 MFMAs.  Grid (tiles of T, G, nseq).  A block whose tile starts
//     at or behind n_s only writes its zeros and leaves before any barrier (as semantic_codes_rows_kernel); in a partly live
//     tile a wave whose 64 frames are all dead skips the MFMAs but keeps the barriers and its share of the B copies.
//     K is walked in one fixed order inside one block, no split-K, no atomics: a row's live frames do not depend on nseq, T
//     or the other rows.
//   Epilogue.  + bias in fp32, GELU (gelu_f of evt_common.h, the function evt_gelu_rows_fwd uses), ONE rounding to the
//     storage type, through a per-wave LDS tile (the dead xs / B space) so that the stores are 16 bytes wide along channels.
//
// Constants (PC_TILE, PC_KC, 4 waves): chosen by the arithmetic above; DESIGN_HISTORY.md has what was measured.
#include "evt_common.h"
#include "../../include/evt.h"

namespace {

constexpr int PC_TILE = EVT_POS_CONV_TILE, PC_WAVES = 4, PC_WM = 64, PC_RT = PC_WM / 16, PC_THREADS = PC_WAVES * 64;
static_assert(PC_TILE == PC_WAVES * PC_WM, "four waves of 64 frames");
constexpr int PC_FRAG = 64 * 8;                                   // elements of one B fragment

typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
__device__ __forceinline__ void pc_glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)l, 16, 0, 0);
}
__device__ __forceinline__ void pc_wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// K steps per B chunk: 12 KiB per chunk at cg = 48 in both types (two buffers = 24 KiB)
template <typename T> struct PcKc;
template <> struct PcKc<h16_t> { static constexpr int v = 4; };
template <> struct PcKc<float> { static constexpr int v = 2; };

template <typename T> constexpr int pc_pitch(int cg) { return sizeof(T) == 2 && (cg / 8) % 4 != 2 ? cg + 16 : cg; }

template <typename T> size_t pc_lds_bytes(int cg, int k) {
  const size_t main = ((size_t)(PC_TILE + k - 1) * pc_pitch<T>(cg) + 2 * (size_t)PcKc<T>::v * (cg / 16) * PC_FRAG) * sizeof(T);
  const size_t epi = (size_t)PC_TILE * (cg + 16 / sizeof(T)) * sizeof(T);
  return main > epi ? main : epi;
}

// one K step of one wave: 4 row tiles x NT column tiles
template <int NT>
__device__ __forceinline__ void pc_step(const h16_t* a, int rt_stride, const h16_t* b, f32x4 (&acc)[PC_RT][NT]) {
  h16x8 af[PC_RT], bf[NT];
#pragma unroll
  for (int rt = 0; rt < PC_RT; ++rt) af[rt] = *reinterpret_cast<const h16x8*>(a + rt * rt_stride);
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) bf[ct] = *reinterpret_cast<const h16x8*>(b + ct * PC_FRAG);
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
#pragma unroll
    for (int rt = 0; rt < PC_RT; ++rt) acc[rt][ct] = EVT_MFMA_16x16x32(af[rt], bf[ct], acc[rt][ct], 0, 0, 0);
}
template <int NT>
__device__ __forceinline__ void pc_step(const float* a, int rt_stride, const float* b, f32x4 (&acc)[PC_RT][NT]) {
  float af[PC_RT][8], bf[NT][8];
#pragma unroll
  for (int rt = 0; rt < PC_RT; ++rt) {
    const float4 lo = *reinterpret_cast<const float4*>(a + rt * rt_stride), hi = *reinterpret_cast<const float4*>(a + rt * rt_stride + 4);
    af[rt][0] = lo.x; af[rt][1] = lo.y; af[rt][2] = lo.z; af[rt][3] = lo.w;
    af[rt][4] = hi.x; af[rt][5] = hi.y; af[rt][6] = hi.z; af[rt][7] = hi.w;
  }
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    const float4 lo = *reinterpret_cast<const float4*>(b + ct * PC_FRAG), hi = *reinterpret_cast<const float4*>(b + ct * PC_FRAG + 4);
    bf[ct][0] = lo.x; bf[ct][1] = lo.y; bf[ct][2] = lo.z; bf[ct][3] = lo.w;
    bf[ct][4] = hi.x; bf[ct][5] = hi.y; bf[ct][6] = hi.z; bf[ct][7] = hi.w;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int rt = 0; rt < PC_RT; ++rt)
        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[rt][i], bf[ct][i], acc[rt][ct], 0, 0, 0);
}

// grid (ceil(Tn / PC_TILE), G, nseq), 256 threads, pc_lds_bytes<T>(CG, k) of dynamic LDS
template <typename T, int CG>
__global__ __launch_bounds__(PC_THREADS) void pos_conv_rows_kernel(const T* __restrict__ x, const int32_t* __restrict__ lens,
                                                                  int Tn, int C, int k, const T* __restrict__ image,
                                                                  const float* __restrict__ bias, int act,
                                                                  T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = CG / 16, P = pc_pitch<T>(CG), KC = PcKc<T>::v;
  constexpr int E = 16 / sizeof(T), SEG = CG / E;               // elements per 16 bytes; 16-byte segments of a frame's group
  constexpr int CHUNK = KC * NT * PC_FRAG;                      // elements of one B buffer
  constexpr int UPS = NT * PC_FRAG * (int)sizeof(T) / 1024;     // 1 KiB copy units (one wave, 16 bytes a lane) per K step
  constexpr int EP = CG + E;                                    // row pitch of the epilogue tile
  const int s = blockIdx.z, g = blockIdx.y, t0 = blockIdx.x * PC_TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), j = lane & 15, q = lane >> 4;
  const int ns = lens ? min(max(lens[s], 0), Tn) : Tn;
  const int tw = min(PC_TILE, Tn - t0);                         // frames of this tile that exist in out (> 0 by the grid)
  const int tl = min(PC_TILE, ns - t0);                         // live frames of this tile (block-uniform; <= 0: none)
  T* orow = out + ((long)s * Tn + t0) * C + g * CG;
  {
    const int z0 = max(tl, 0);
    for (int i = tid; i < (tw - z0) * SEG; i += PC_THREADS) {
      const int f = z0 + i / SEG, sg = i % SEG;
      *reinterpret_cast<uint4*>(orow + (long)f * C + sg * E) = make_uint4(0u, 0u, 0u, 0u);
    }
  }
  if (tl <= 0) return;                                          // the whole block: no barrier is left waiting

  const int NF = PC_TILE + k - 1;
  T* bs = reinterpret_cast<T*>(smem);                           // [2][CHUNK]: in front, the LDS-DMA targets stay below 64 KB
  T* xs = bs + 2 * CHUNK;                                       // [NF][P]
  const int KS = k * CG / 32, nchunk = (KS + KC - 1) / KC;
  const T* img = image + (long)g * KS * NT * PC_FRAG;
  // chunk c -> buffer c & 1: whole 1 KiB units of the K steps that exist, so nothing behind the group's image is read
  auto issue = [&](int c) {
    const int units = min(KC, KS - c * KC) * UPS;
    const char* src = reinterpret_cast<const char*>(img + (long)c * CHUNK) + lane * 16;
    char* dst = reinterpret_cast<char*>(bs + (c & 1) * CHUNK);
    for (int u = wave; u < units; u += PC_WAVES) pc_glds16(src + u * 1024, dst + u * 1024);
  };
  issue(0);
  {
    // frames t0 - k / 2 .. t0 - k / 2 + NF - 1 of the row; zeros outside [0, ns)
    const T* xrow = x + (long)s * Tn * C + g * CG;
    const int f0 = t0 - k / 2;
    for (int i = tid; i < NF * SEG; i += PC_THREADS) {
      const int fi = i / SEG, sg = i - fi * SEG, f = f0 + fi;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (f >= 0 && f < ns) v = *reinterpret_cast<const uint4*>(xrow + (long)f * C + sg * E);
      *reinterpret_cast<uint4*>(xs + fi * P + sg * E) = v;
    }
  }
  pc_wait_vm0();
  __syncthreads();

  f32x4 acc[PC_RT][NT];
#pragma unroll
  for (int rt = 0; rt < PC_RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool wlive = wave * PC_WM < tl;                         // per wave
  const T* arow = xs + (wave * PC_WM + j) * P;                  // row m = wave * 64 + rt * 16 + j of the view
  for (int c = 0; c < nchunk; ++c) {
    if (c + 1 < nchunk) issue(c + 1);                           // its buffer was last read before the previous barrier
    if (wlive) {
      const T* bb = bs + (c & 1) * CHUNK + lane * 8;
#pragma unroll
      for (int si = 0; si < KC; ++si) {
        const int ks = c * KC + si;
        if (ks < KS) {
          const int kk = ks * 32 + q * 8;
          pc_step<NT>(arow + kk + (kk / CG) * (P - CG), 16 * P, bb + si * NT * PC_FRAG, acc);
        }
      }
    }
    pc_wait_vm0();
    __syncthreads();
  }

  // every wave is behind the last barrier and no copy is in flight: xs / bs are dead, the waves' output tiles take their place
  if (!wlive) return;
  T* es = reinterpret_cast<T*>(smem) + wave * PC_WM * EP;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    const float bv = bias ? bias[g * CG + ct * 16 + j] : 0.f;
#pragma unroll
    for (int rt = 0; rt < PC_RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = acc[rt][ct][r] + bv;
        es[(rt * 16 + q * 4 + r) * EP + ct * 16 + j] = from_f<T>(act ? gelu_f(v) : v);
      }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // the wave reads back what its own lanes wrote
  const int rows = min(PC_WM, tl - wave * PC_WM);
  T* ow = orow + (long)wave * PC_WM * C;
  for (int i = lane; i < rows * SEG; i += 64) {
    const int r = i / SEG, sg = i - r * SEG;
    *reinterpret_cast<uint4*>(ow + (long)r * C + sg * E) = *reinterpret_cast<const uint4*>(es + r * EP + sg * E);
  }
}

template <typename T>
__global__ void pos_conv_pack_kernel(const float* __restrict__ w, int cg, int k, long n, T* __restrict__ image) {
  const int NT = cg / 16, KS = k * cg / 32;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
    const int i = (int)(idx & 7), lane = (int)(idx >> 3) & 63, j = lane & 15, q = lane >> 4;
    long rest = idx >> 9;
    const int ct = (int)(rest % NT);
    rest /= NT;
    const int ks = (int)(rest % KS), g = (int)(rest / KS);
    const int kk = 32 * ks + 8 * q + i, tap = kk / cg, c = kk - tap * cg;
    image[idx] = from_f<T>(w[((long)(g * cg + ct * 16 + j) * cg + c) * k + tap]);
  }
}

template <typename T, int CG>
int pc_launch(const void* x, const int32_t* lens, int nseq, int Tn, int C, int G, int k, const void* image, const float* bias,
              int act, void* out, hipStream_t stream) {
  static size_t have = 48 * 1024;
  const size_t lds = pc_lds_bytes<T>(CG, k);
  if (lds > have) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&pos_conv_rows_kernel<T, CG>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return EVT_ELAUNCH;
    have = lds;
  }
  const dim3 grid((Tn + PC_TILE - 1) / PC_TILE, G, nseq);
  hipLaunchKernelGGL((pos_conv_rows_kernel<T, CG>), grid, dim3(PC_THREADS), lds, stream, (const T*)x, lens, Tn, C, k,
                     (const T*)image, bias, act, (T*)out);
  return evt_check_launch();
}

template <typename T>
int pc_dispatch(int cg, const void* x, const int32_t* lens, int nseq, int Tn, int C, int G, int k, const void* image,
                const float* bias, int act, void* out, hipStream_t stream) {
  switch (cg) {
    case 16: return pc_launch<T, 16>(x, lens, nseq, Tn, C, G, k, image, bias, act, out, stream);
    case 32: return pc_launch<T, 32>(x, lens, nseq, Tn, C, G, k, image, bias, act, out, stream);
    case 48: return pc_launch<T, 48>(x, lens, nseq, Tn, C, G, k, image, bias, act, out, stream);
    case 64: return pc_launch<T, 64>(x, lens, nseq, Tn, C, G, k, image, bias, act, out, stream);
  }
  return EVT_ENOTSUP;
}

// the shapes both entry points serve
int pc_shape(int32_t dtype, int32_t C, int32_t G, int32_t k) {
  if (C <= 0 || G <= 0 || k <= 0) return EVT_EINVAL;
  if (dtype != EVT_DT_F32 && dtype != EVT_DT_HALF) return EVT_ENOTSUP;
  if (C % G) return EVT_ENOTSUP;
  const int cg = C / G;
  if (cg != 16 && cg != 32 && cg != 48 && cg != 64) return EVT_ENOTSUP;
  if (k < 2 || k > 128 || (k * cg) % 32) return EVT_ENOTSUP;
  return EVT_OK;
}

}  // namespace

extern "C" int evt_pos_conv_pack(int32_t dtype, const float* w, int32_t C, int32_t G, int32_t k, void* image, void* stream) {
  if (!w || !image) return EVT_EINVAL;
  if (const int rc = pc_shape(dtype, C, G, k)) return rc;
  if (((uintptr_t)w | (uintptr_t)image) & 15) return EVT_EINVAL;
  const int cg = C / G;
  const long n = (long)C * cg * k;
  const int blocks = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
  evt_set_last_tag(dtype == EVT_DT_F32 ? "pos_conv_pack<f32>" : "pos_conv_pack<" EVT_HALF_NAME ">");
  if (dtype == EVT_DT_F32)
    hipLaunchKernelGGL(pos_conv_pack_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, cg, k, n, (float*)image);
  else
    hipLaunchKernelGGL(pos_conv_pack_kernel<h16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, cg, k, n, (h16_t*)image);
  return evt_check_launch();
}

extern "C" int evt_pos_conv_rows(int32_t dtype, const void* x, const int32_t* lens, int32_t nseq, int32_t T, int32_t C,
                                 int32_t G, int32_t k, const void* image, const float* bias, int32_t act, void* out,
                                 void* stream) {
  if (!x || !image || !out) return EVT_EINVAL;
  if (nseq <= 0 || nseq > 65535 || T <= 0) return EVT_EINVAL;
  if (const int rc = pc_shape(dtype, C, G, k)) return rc;
  if (act != 0 && act != 1) return EVT_ENOTSUP;
  if (((uintptr_t)x | (uintptr_t)image | (uintptr_t)out | (uintptr_t)bias) & 15) return EVT_EINVAL;
  const int cg = C / G;
  evt_set_last_tag(dtype == EVT_DT_F32 ? "pos_conv_rows<f32,cg%d,k%d>" : "pos_conv_rows<" EVT_HALF_NAME ",cg%d,k%d>", cg, k);
  if (dtype == EVT_DT_F32)
    return pc_dispatch<float>(cg, x, lens, nseq, T, C, G, k, image, bias, act, out, (hipStream_t)stream);
  return pc_dispatch<h16_t>(cg, x, lens, nseq, T, C, G, k, image, bias, act, out, (hipStream_t)stream);
}

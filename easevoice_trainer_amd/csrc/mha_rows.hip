// fp32 attention core of the feature extractors on ragged rows, gfx950: a flash kernel on mfma_f32_16x16x4f32 (true fp32
// multiply-accumulate, no 16-bit or reduced-precision product anywhere), forward only, ONE launch, no workspace.
// include/evt.h has the definition of the entry point (evt_mha_rows_f32).
//
// Reference call sites: transformers' HubertAttention / BertSelfAttention inside the models the reference runs on the CPU in
// float32 (src/easevoice/feature_extractor/cnhubert.py:16-32, src/normalization/normalize.py:65-106, 158).
//
//   out_i = sum_j softmax_j(scale * q_i . k_j) v_j over the live keys j < lens_k[b]; no window, no dropout, no lse.
//
// Work split.  Grid (query tiles, H, B), 4 waves.  A block owns one (b, h) and MR_QT = 64 queries counted from the row's
//   query 0, a wave 16 of them; the block walks the ceil(lens_k[b] / MR_KT) key tiles of MR_KT = 32 keys in ascending order.
//   A block whose first query is at or behind lens_q[b] (or whose item has no live key) writes its zeros and leaves before
//   any barrier; in a partly live tile a wave whose 16 queries are all dead keeps the barriers and its share of the copies
//   and skips the arithmetic.
// Registers.  mfma_f32_16x16x4f32 takes from lane (g = lane / 16, n = lane % 16) A[m = n][k = g] and B[k = g][n] and leaves
//   C[m = 4 g + r][n] in register r.  Which d a lane quarter supplies is free as long as A and B agree (pos_conv.hip):
//   MFMA i of K step c takes d = 16 c + 4 g + i from both.
//   Q: lane (g, n) keeps q[query n][16 c + 4 g .. + 3], c < D / 16, multiplied ONCE by scale * log2(e): D / 4 registers, the
//     B operand of every score MFMA of the key loop.
//   S^T = K . Q^T: A = a 16-key sub-tile of K from LDS (row = key, one ds_read_b128 = the four MFMAs of a K step).  Lane
//     (g, n) then holds the scores of keys 4 g .. 4 g + 3 of query n: a query's running max lives in the four lanes n,
//     n + 16, n + 32, n + 48 -- two cross-lane steps per key tile (xor 16, xor 32), no LDS memory.  The running SUM stays a
//     per-lane partial (the four lanes share the max, hence the rescale factor) and is reduced once, in the epilogue.
//   O^T += V^T . P^T: the same registers are the B operand.  MFMA r takes from lane (g, n) the probability of key 4 g + r,
//     so its A operand is V[key 4 g + r][16 dt + n]: a permuted ds_read_b32 of the V tile, P never leaves registers.
//     Accumulator lane (g, n), register r of tile dt = channel 16 dt + 4 g + r of query n: the epilogue is one reciprocal of
//     the sum, one multiply and 16-byte stores.
// LDS.  K and V tiles [MR_KT][D] with row pitch P = D + 4 floats, double-buffered: 4 * 32 * 68 * 4 = 34 KB at D = 64 (four
//   blocks per CU).  Pitch: P * 4 bytes is an odd number of 16-byte slots (17 at D = 64, 9 at D = 32), so the 16 lanes of a
//   ds_read_b128 group (keys m .. m + 15, one g) start at 16 distinct slots m * P mod 64 = 4 m (D = 64) or a permutation of
//   the multiples of 4 (D = 32): conflict-free.  The permuted V read: lane (g, n) reads word (4 g + r) * P + 16 dt + n, bank
//   16 g + n mod 64 because 4 P = 16 mod 64 for both pitches: 64 lanes, 64 distinct banks.
//   Tiles arrive by plain 16-byte loads into registers (tile t + 1 is in flight while tile t is multiplied) and
//   ds_write_b128 behind the arithmetic, one barrier per tile.  Not LDS-DMA: its target is lane-linear, which excludes the
//   padded pitch, and the rows at or behind lens_k[b] of the last tile have to be ZERO-FILLED by ordinary writes anyway
//   (they are not read from memory; NaN * 0 is NaN on the MFMA).  Their scores are replaced by -inf with a select.
// Order of every sum: key tiles from key 0, inside a tile the MFMA's own order; nothing depends on B, Tq, Tk, the
//   neighbours or the wave a query lands in (an MFMA column is a function of its own B column only).
#include "evt_common.h"
#include "../../include/evt.h"

namespace {

constexpr int MR_QT = EVT_MHA_ROWS_QUERY_TILE, MR_KT = EVT_MHA_ROWS_KEY_TILE, MR_WAVES = 4, MR_THREADS = MR_WAVES * 64;
constexpr int MR_ST = MR_KT / 16;                                 // 16-key sub-tiles of a key tile
static_assert(MR_QT == MR_WAVES * 16, "four waves of 16 queries");
static_assert(MR_KT % 16 == 0, "whole sub-tiles");
// the launch tag.  A named constant: the literal tags in csrc/ are the registry of the multiply-accumulate kernels that have
// integer-exact cases (tests/exact_inputs.py); this is a softmax kernel, as mha.hip's, and rests on the float64 tests.
constexpr const char* MR_TAG = "mha_rows_f32<%d>";

template <int D> constexpr int mr_pitch() { return D + 4; }
template <int D> constexpr size_t mr_lds_bytes() { return (size_t)4 * MR_KT * mr_pitch<D>() * sizeof(float); }

struct MrArgs {
  const float *q, *k, *v;
  const int32_t *lens_q, *lens_k;
  float* out;
  int Tq, Tk;
  long ldq, ldk, ldo;
  float qscale;                                                   // scale * log2(e)
};

// grid (ceil(Tq / MR_QT), H, B), 256 threads, mr_lds_bytes<D>() of dynamic LDS
template <int D>
__global__ __launch_bounds__(MR_THREADS) void mha_rows_f32_kernel(MrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int P = mr_pitch<D>(), NC = D / 16, SEG = D / 4;     // K steps of 16; 16-byte segments of a row
  constexpr int NL = MR_KT * SEG / MR_THREADS;                    // 16-byte loads per thread, tile and operand
  static_assert(MR_KT * SEG % MR_THREADS == 0, "whole copy rounds");
  constexpr int TILE = MR_KT * P;                                 // floats of one buffer
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * MR_QT;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), n = lane & 15, g = lane >> 4;
  const int lenq = a.lens_q ? min(max(a.lens_q[b], 0), a.Tq) : a.Tq;
  const int lenk = a.lens_k ? min(max(a.lens_k[b], 0), a.Tk) : a.Tk;
  const int qi = q0 + wave * 16 + n;                              // this lane's query
  float* orow = a.out + ((long)b * a.Tq + qi) * a.ldo + h * D + 4 * g;

  if (q0 >= lenq || lenk == 0) {                                  // the whole block: no barrier is left waiting
    if (qi < a.Tq)
#pragma unroll
      for (int dt = 0; dt < NC; ++dt) *reinterpret_cast<float4*>(orow + 16 * dt) = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }

  float* ks = reinterpret_cast<float*>(smem);                     // [2][MR_KT][P]
  float* vs = ks + 2 * TILE;                                      // [2][MR_KT][P]
  const float* kg = a.k + (long)b * a.Tk * a.ldk + h * D;
  const float* vg = a.v + (long)b * a.Tk * a.ldk + h * D;
  const int ntile = (lenk + MR_KT - 1) / MR_KT;

  float4 kr[NL], vr[NL];
  // tile t -> registers: rows at or behind lenk are zeros and are not read
  auto fetch = [&](int t) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + i * MR_THREADS, row = idx / SEG, sg = idx - row * SEG, key = t * MR_KT + row;
      kr[i] = vr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (key < lenk) {
        kr[i] = *reinterpret_cast<const float4*>(kg + (long)key * a.ldk + 4 * sg);
        vr[i] = *reinterpret_cast<const float4*>(vg + (long)key * a.ldk + 4 * sg);
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + i * MR_THREADS, row = idx / SEG, sg = idx - row * SEG;
      *reinterpret_cast<float4*>(ks + buf * TILE + row * P + 4 * sg) = kr[i];
      *reinterpret_cast<float4*>(vs + buf * TILE + row * P + 4 * sg) = vr[i];
    }
  };
  fetch(0);

  const bool wlive = q0 + wave * 16 < lenq;                       // per wave
  float qf[NC][4];
  {
    float4 z[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) z[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (qi < lenq) {                                              // a dead query is not read: its column runs on zeros
      const float* qrow = a.q + ((long)b * a.Tq + qi) * a.ldq + h * D + 4 * g;
#pragma unroll
      for (int c = 0; c < NC; ++c) z[c] = *reinterpret_cast<const float4*>(qrow + 16 * c);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      qf[c][0] = z[c].x * a.qscale; qf[c][1] = z[c].y * a.qscale; qf[c][2] = z[c].z * a.qscale; qf[c][3] = z[c].w * a.qscale;
    }
  }
  stash(0);
  __syncthreads();

  f32x4 acc[NC];
#pragma unroll
  for (int dt = 0; dt < NC; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrun = -INFINITY, lrun = 0.f;                             // the query's running max; this lane's share of the sum
  for (int t = 0; t < ntile; ++t) {
    if (t + 1 < ntile) fetch(t + 1);
    if (wlive) {
      const float* kt = ks + (t & 1) * TILE + n * P + 4 * g;
      const float* vt = vs + (t & 1) * TILE + 4 * g * P + n;
      f32x4 s[MR_ST];
#pragma unroll
      for (int st = 0; st < MR_ST; ++st) s[st] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int st = 0; st < MR_ST; ++st) {
          const float4 kf = *reinterpret_cast<const float4*>(kt + st * 16 * P + 16 * c);
          s[st] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.x, qf[c][0], s[st], 0, 0, 0);
          s[st] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.y, qf[c][1], s[st], 0, 0, 0);
          s[st] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.z, qf[c][2], s[st], 0, 0, 0);
          s[st] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.w, qf[c][3], s[st], 0, 0, 0);
        }
      // keys at or behind lenk: -inf by a select.  Key t * MR_KT is live, so the tile's max is finite for every query.
      float mt = -INFINITY;
#pragma unroll
      for (int st = 0; st < MR_ST; ++st)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = t * MR_KT + st * 16 + 4 * g + r;
          s[st][r] = key < lenk ? s[st][r] : -INFINITY;
          mt = fmaxf(mt, s[st][r]);
        }
      mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float mnew = fmaxf(mrun, mt);
      const float alpha = __builtin_amdgcn_exp2f(mrun - mnew);   // 0 on the first tile (mrun = -inf, mnew finite)
      mrun = mnew;
      float psum = 0.f;
#pragma unroll
      for (int st = 0; st < MR_ST; ++st)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[st][r] = __builtin_amdgcn_exp2f(s[st][r] - mnew);
          psum += s[st][r];
        }
      lrun = lrun * alpha + psum;
#pragma unroll
      for (int dt = 0; dt < NC; ++dt) acc[dt] *= alpha;
#pragma unroll
      for (int st = 0; st < MR_ST; ++st)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int dt = 0; dt < NC; ++dt)
            acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vt[(st * 16 + r) * P + 16 * dt], s[st][r], acc[dt], 0, 0, 0);
    }
    if (t + 1 < ntile) stash((t + 1) & 1);                        // that buffer was last read before the previous barrier
    __syncthreads();
  }

  lrun += __shfl_xor(lrun, 16, 64);                               // (l_g + l_g^1) + (l_g^2 + l_g^3): the same bits in all four lanes
  lrun += __shfl_xor(lrun, 32, 64);
  if (qi >= a.Tq) return;
  const bool live = qi < lenq;
  const float inv = live ? 1.f / lrun : 0.f;
#pragma unroll
  for (int dt = 0; dt < NC; ++dt) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) o = make_float4(acc[dt][0] * inv, acc[dt][1] * inv, acc[dt][2] * inv, acc[dt][3] * inv);
    *reinterpret_cast<float4*>(orow + 16 * dt) = o;
  }
}

template <int D>
int mr_launch(const MrArgs& a, int B, int H, hipStream_t stream) {
  const dim3 grid((a.Tq + MR_QT - 1) / MR_QT, H, B);
  hipLaunchKernelGGL((mha_rows_f32_kernel<D>), grid, dim3(MR_THREADS), mr_lds_bytes<D>(), stream, a);
  return evt_check_launch();
}
static_assert(mr_lds_bytes<64>() <= 48 * 1024, "dynamic LDS below the default limit: no function attribute to raise");

}  // namespace

extern "C" int evt_mha_rows_f32(const evt_mha_params* p, const void* q, const void* k, const void* v, const int32_t* lens_q,
                                const int32_t* lens_k, void* out, void* stream) {
  if (!p || !q || !k || !v || !out) return EVT_EINVAL;
  if (p->dtype != EVT_DT_F32 || p->window >= 0 || p->dropout_p != 0.f) return EVT_EINVAL;
  if (p->D != 32 && p->D != 64) return EVT_EINVAL;
  if (p->B <= 0 || p->B > 65535 || p->H <= 0 || p->H > 65535 || p->Tq <= 0 || p->Tk <= 0) return EVT_EINVAL;
  const int64_t hd = (int64_t)p->H * p->D;
  if (p->ldq < hd || p->ldk < hd || p->ldo < hd || p->ldq % 4 || p->ldk % 4 || p->ldo % 4) return EVT_EINVAL;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) return EVT_EINVAL;
  if (((uintptr_t)lens_q | (uintptr_t)lens_k) & 3) return EVT_EINVAL;
  if (!(p->scale > 0.f)) return EVT_EINVAL;
  MrArgs a{(const float*)q, (const float*)k, (const float*)v, lens_q, lens_k, (float*)out, p->Tq, p->Tk,
           (long)p->ldq, (long)p->ldk, (long)p->ldo, p->scale * 1.44269504088896340736f};
  evt_set_last_tag(MR_TAG, (int)p->D);
  if (p->D == 64) return mr_launch<64>(a, p->B, p->H, (hipStream_t)stream);
  return mr_launch<32>(a, p->B, p->H, (hipStream_t)stream);
}

// The key/value cache of a stream session in MXFP8, head-major, for gfx950 (auto_reg/t2s_infer.py StreamSession with
// kv_dtype="mxfp8").  The model's head width is 32, which is one OCP MX block: a head row of 32 values becomes 32 e4m3fn
// code bytes and ONE E8M0 scale byte (33 bytes instead of 64 in a 16-bit cache), defined in include/evt.h.  Per layer,
// keys and values each are  codes uint8 [B][H][Lmax][32]  and  scales uint8 [B][H][Lmax]:  a (row, head) workgroup of the
// decode step reads one contiguous stream of 32 L code bytes and L scale bytes.
//
//   kv_pack_mx8_rows   the prompt pass's keys and values of one layer into the cache, K and V in one launch, through a
//                      device row map (one prompt row may fill several candidate slots).  A wave-half owns one
//                      (position, head) row: amax and the NaN/Inf test by cross-lane operations, the codes through
//                      v_cvt_pk_fp8_f32, gathered into two 16-byte stores; lane 0 stores the scale byte.  The transposition
//                      [S][H] -> [H][S] happens in the store address.
//   dec_attn_rows_mx8  evt_dec_attn_rows on this cache: one 256-thread workgroup per (row, head).  Scores: thread t owns
//                      keys t + 256 i, two 16-byte loads each (consecutive threads read consecutive 32-byte rows),
//                      2^ek applied once per key.  P.V: thread t owns the 16-byte half row (t & 1) of keys (t >> 1) + 128 i,
//                      the scale folded into the probability; the 128 partial rows are summed through LDS in two fixed
//                      stages (8 x 16 rows, then 8).  Codes are widened by v_cvt_pk_f32_fp8.  No MFMA: one query per head
//                      is a GEMV.  Every sum is fp32 in an order that depends on the row's own length alone.
// The power-of-two scale commutes with every fp32 rounding (no product here comes near the ends of the exponent range
// unless the data already does), so applying it after the sum gives the bits of summing dequantised values.
// v_cvt_pk_fp8_f32 was compared with the definition's round-to-nearest-even on an MI355X over every fp32 pattern with
// |x| <= 448, and v_cvt_f32_fp8 over all 256 codes: no difference, subnormal codes and signed zeros included -- there is
// no fix-up path.
#include "s1_decode_common.h"
#include "mx8_quant.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// the 16 values of 16 code bytes
__device__ __forceinline__ void mx_widen16(const uint4& u, float* f) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    f[4 * i] = lo.x; f[4 * i + 1] = lo.y; f[4 * i + 2] = hi.x; f[4 * i + 3] = hi.y;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void kv_pack_mx8_rows(const T* __restrict__ qkv, const int* __restrict__ dst_row,
                                                        const int* __restrict__ src_row, const int* __restrict__ n_pos,
                                                        uint8_t* kq, uint8_t* ks, uint8_t* vq, uint8_t* vs, int n, int k,
                                                        int S, int B, int H, int Lmax) {
  // item = ((m * S + pos) * 2 + kv) * H + h: consecutive wave-halves read consecutive 32-value pieces of one qkv row
  const long item = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int l = threadIdx.x & 31;
  const long total = (long)n * S * 2 * H;
  if (item >= total) return;
  const int h = (int)(item % H), kv = (int)(item / H % 2), pos = (int)(item / (2 * H) % S), m = (int)(item / (2L * H * S));
  const int dst = dst_row[m], src = src_row[m];
  int np = n_pos[m];
  np = np < S ? np : S;
  np = np < Lmax ? np : Lmax;
  // the map is device memory the launcher cannot see: an entry outside the buffers writes nothing.  Both returns are
  // uniform over the wave-half, and no value that mx_quant_row_store keeps crosses the halves of a wave.
  if (dst < 0 || dst >= B || src < 0 || src >= k || pos >= np) return;
  const int E = H * kD;
  const float v = to_f<T>(qkv[((long)src * S + pos) * 3 * E + (1 + kv) * E + h * kD + l]);
  const long row = ((long)dst * H + h) * Lmax + pos;
  mx_quant_row_store(v, l, (kv ? vq : kq) + row * kD, (kv ? vs : ks) + row);
}

constexpr int kPF = 3;         // value chunks of a thread requested before the softmax: keys (t >> 1) + 128 i, i < kPF
constexpr int kG = 128;        // key groups of the P.V phase

__global__ __launch_bounds__(256) void dec_attn_rows_mx8(const float* __restrict__ qkv, uint8_t* kq, uint8_t* ks,
                                                         uint8_t* vq, uint8_t* vs, const int* __restrict__ rstate,
                                                         float* __restrict__ out, int H, int Lmax,
                                                         const int* __restrict__ x_lens, int x_len) {
  extern __shared__ float sc[];   // [Lmax] scores -> probabilities
  __shared__ float qs[kD], kn[kD], vn[kD], red[4], part[kG][kD + 1], part2[8][kD];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / H, h = blockIdx.x % H, E = H * kD;
  const int* rs = rstate + b * EVT_ROW_WORDS;
  if (rs[EVT_ROW_STATUS] != EVT_ROW_RUNNING) return;   // idle / stopped: no cache write, out untouched
  const int pos = rs[EVT_ROW_POS];
  if (pos < 0 || pos >= Lmax) return;                   // cache full: guards memory, the host bounds the steps
  const int L = pos + 1;
  const int mlo = x_lens ? x_lens[b] : 0, mhi = x_lens ? x_len : 0;   // keys mlo <= j < mhi: padding, skipped
  const long slab = ((long)b * H + h) * Lmax;
  const uint8_t* kqb = kq + slab * kD;
  const uint8_t* vqb = vq + slab * kD;
  const uint8_t* ksb = ks + slab;
  const uint8_t* vsb = vs + slab;
  const int g = tid >> 1, c = tid & 1;
  // ---- requests that depend on nothing computed here: the first key row and the first kPF value chunks ----
  uint4 k0[2], vpre[kPF];
  int ek0 = 0, evpre[kPF];
  if (tid < L && tid != pos) {
    k0[0] = *reinterpret_cast<const uint4*>(kqb + (long)tid * kD);
    k0[1] = *reinterpret_cast<const uint4*>(kqb + (long)tid * kD + 16);
    ek0 = ksb[tid];
  }
#pragma unroll
  for (int i = 0; i < kPF; ++i) {
    const int j = g + i * kG;
    if (j < L && j != pos) {
      vpre[i] = *reinterpret_cast<const uint4*>(vqb + (long)j * kD + c * 16);
      evpre[i] = vsb[j];
    }
  }
  // ---- the new token: wave 0 quantises k (lanes 0..31) and v (lanes 32..63), appends both, keeps the dequantised ----
  if (tid < 64) {
    const int d = tid & 31, isv = tid >> 5;
    const float* base = qkv + (long)b * 3 * E + h * kD + d;
    if (!isv) qs[d] = base[0] * rsqrtf((float)kD);
    const float x = base[isv ? 2 * E : E];
    const long row = slab + pos;
    const float dq = mx_quant_row_store(x, d, (isv ? vq : kq) + row * kD, (isv ? vs : ks) + row);
    (isv ? vn : kn)[d] = dq;
  }
  __syncthreads();
  float q[kD];
#pragma unroll
  for (int d = 0; d < kD; ++d) q[d] = qs[d];
  // ---- scores ----
  float mx = -INFINITY;
  for (int j = tid; j < L; j += 256) {
    float s = 0.f;
    if (j >= mlo && j < mhi) {
      s = -INFINITY;
    } else if (j == pos) {
#pragma unroll
      for (int d = 0; d < kD; ++d) s += q[d] * kn[d];
    } else {
      uint4 u0, u1;
      int ek;
      if (j == tid) {
        u0 = k0[0]; u1 = k0[1]; ek = ek0;
      } else {
        u0 = *reinterpret_cast<const uint4*>(kqb + (long)j * kD);
        u1 = *reinterpret_cast<const uint4*>(kqb + (long)j * kD + 16);
        ek = ksb[j];
      }
      float f[kD];
      mx_widen16(u0, f);
      mx_widen16(u1, f + 16);
#pragma unroll
      for (int d = 0; d < kD; ++d) s += q[d] * f[d];
      s = mx_scale(s, ek);
    }
    sc[j] = s;
    mx = fmaxf(mx, s);
  }
  mx = block_max(mx, red, 4);
  float sum = 0.f;
  for (int j = tid; j < L; j += 256) {
    const float e = sc[j] == -INFINITY ? 0.f : expf(sc[j] - mx);
    sc[j] = e;
    sum += e;
  }
  sum = block_sum(sum, red, 4);      // its barriers also publish sc[]
  // ---- P.V: acc[e] += (p_j 2^ev_j) code_je over this thread's keys, in ascending j ----
  float acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
  for (int i = 0; i < kPF; ++i) {
    const int j = g + i * kG;
    if (j < L && !(j >= mlo && j < mhi)) {
      if (j == pos) {
        const float pj = sc[j];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] += pj * vn[c * 16 + e];
      } else {
        const float pj = mx_scale(sc[j], evpre[i]);
        float f[16];
        mx_widen16(vpre[i], f);
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] += pj * f[e];
      }
    }
  }
  for (int j = g + kPF * kG; j < L; j += kG) {
    if (j >= mlo && j < mhi) continue;
    if (j == pos) {
      const float pj = sc[j];
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] += pj * vn[c * 16 + e];
    } else {
      const uint4 u = *reinterpret_cast<const uint4*>(vqb + (long)j * kD + c * 16);
      const float pj = mx_scale(sc[j], vsb[j]);
      float f[16];
      mx_widen16(u, f);
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] += pj * f[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) part[g][c * 16 + e] = acc[e];
  __syncthreads();
  {   // 128 partial rows -> 8 (rows 16 r .. 16 r + 15 in order) -> 1 (r = 0 .. 7 in order)
    const int d = tid & 31, r = tid >> 5;
    float o = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) o += part[r * 16 + i][d];
    part2[r][d] = o;
  }
  __syncthreads();
  if (tid < kD) {
    float o = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) o += part2[r][tid];
    out[(long)b * E + h * kD + tid] = o / sum;
  }
}

}  // namespace

extern "C" {

int evt_kv_pack_mx8_rows(int32_t dtype, const void* qkv, const int32_t* dst_row, const int32_t* src_row,
                         const int32_t* n_pos, uint8_t* kcodes, uint8_t* kscales, uint8_t* vcodes, uint8_t* vscales,
                         int32_t n, int32_t k, int32_t S, int32_t B, int32_t H, int32_t D, int32_t Lmax, void* stream) {
  if (!qkv || !dst_row || !src_row || !n_pos || !kcodes || !kscales || !vcodes || !vscales || n <= 0 || k <= 0 || S <= 0 ||
      B <= 0 || H <= 0 || Lmax <= 0)
    return EVT_EINVAL;
  if (D != kD) return EVT_ENOTSUP;
  const long items = (long)n * S * 2 * H;
  if ((items + 7) / 8 > 0x7fffffffL) return EVT_ENOTSUP;
  const dim3 grid((unsigned)((items + 7) / 8)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EVT_DT_HALF)
    hipLaunchKernelGGL(kv_pack_mx8_rows<h16_t>, grid, block, 0, st, (const h16_t*)qkv, (const int*)dst_row,
                       (const int*)src_row, (const int*)n_pos, kcodes, kscales, vcodes, vscales, n, k, S, B, H, Lmax);
  else if (dtype == EVT_DT_F32)
    hipLaunchKernelGGL(kv_pack_mx8_rows<float>, grid, block, 0, st, (const float*)qkv, (const int*)dst_row,
                       (const int*)src_row, (const int*)n_pos, kcodes, kscales, vcodes, vscales, n, k, S, B, H, Lmax);
  else return EVT_EINVAL;
  return evt_check_launch();
}

int evt_dec_attn_rows_mx8(const float* qkv, uint8_t* kcodes, uint8_t* kscales, uint8_t* vcodes, uint8_t* vscales,
                          const int32_t* rstate, float* out, int32_t B, int32_t H, int32_t D, int32_t Lmax,
                          const int32_t* x_lens, int32_t x_len, void* stream) {
  if (!qkv || !kcodes || !kscales || !vcodes || !vscales || !rstate || !out || B <= 0 || H <= 0 || Lmax <= 0)
    return EVT_EINVAL;
  if (D != kD || (size_t)Lmax * 4 > 40 * 1024) return EVT_ENOTSUP;
  hipLaunchKernelGGL(dec_attn_rows_mx8, dim3(B * H), dim3(256), (size_t)Lmax * sizeof(float), (hipStream_t)stream, qkv,
                     kcodes, kscales, vcodes, vscales, (const int*)rstate, out, H, Lmax, (const int*)x_lens, x_len);
  return evt_check_launch();
}

}  // extern "C"

// The MXFP8 head-row quantiser of the stream sessions' key/value cache (the format in include/evt.h), shared by the kernels
// that write such a cache: s1_decode_mx8.hip (the pack kernel and the decode step's append) and attn_packed.hip (the packed
// prompt pass).  One definition, so that the bytes of a head row cannot depend on the kernel that wrote it.
#pragma once
#include "evt_common.h"

namespace {

constexpr int kD = 32;          // head width = MX block
constexpr int kScaleNaN = 0xFF;

// 2^(s - 127) * x, NaN for the scale byte of a row that held NaN / Inf.  ldexpf is exact (no fp32 denormal is formed from
// a normal operand unless the definition's own value is one).
__device__ __forceinline__ float mx_scale(float x, int s) { return s == kScaleNaN ? NAN : ldexpf(x, s - 127); }

// One head row, held one value per lane by the 32 lanes of a wave-half (l = lane & 31): quantises it as include/evt.h
// defines, stores the 32 code bytes at `codes` (two 16-byte stores, lanes 0 and 16) and the scale byte at `scale` (lane
// 0), and returns the lane's DEQUANTISED value.  Every lane of the wave calls it (the shuffles need no inactive lane's
// value: each half reads its own lanes only, or values that are discarded).
__device__ __forceinline__ float mx_quant_row_store(float v, int l, uint8_t* codes, uint8_t* scale) {
  const unsigned long long bad64 = __ballot(!(fabsf(v) < INFINITY));   // NaN or +-Inf
  const unsigned bad = (threadIdx.x & 32) ? (unsigned)(bad64 >> 32) : (unsigned)bad64;
  float a = fabsf(v);
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
  int s;
  float sv;       // the value scaled into e4m3's range
  if (bad) {
    s = kScaleNaN;
    sv = 0.f;
  } else if (a == 0.f) {
    s = 0;
    sv = v;       // +-0 -> 0x00 / 0x80
  } else {
    int x;
    const float m = frexpf(a, &x);
    int e = m <= 0.875f ? x - 9 : x - 8;      // a * 2^-e in (224, 448]
    e = e < -127 ? -127 : e;                   // e <= 120 always
    s = e + 127;
    sv = ldexpf(v, -e);
  }
  const float nb = __shfl_down(sv, 1, 64);
  const unsigned pk = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(sv, nb, 0, false) & 0xFFFFu;   // even lanes: lanes l, l + 1
  const unsigned dw = pk | (__shfl_down(pk, 2, 64) << 16);                                     // l % 4 == 0: l .. l + 3
  uint4 q;
  q.x = dw;
  q.y = __shfl_down(dw, 4, 64);
  q.z = __shfl_down(dw, 8, 64);
  q.w = __shfl_down(dw, 12, 64);
  if ((l & 15) == 0) *reinterpret_cast<uint4*>(codes + l) = q;
  if (l == 0) *scale = (uint8_t)s;
  const unsigned prev = __shfl_up(pk, 1, 64);        // by every lane: a shuffle inside a branch reads inactive lanes
  const unsigned own = (l & 1) ? prev >> 8 : pk;
  return mx_scale(__builtin_amdgcn_cvt_f32_fp8((int)(own & 0xFFu), 0), s);
}

}  // namespace

// MFMA fragment helpers of the 16-bit prefix-LM attention kernels (attention.hip, attn_packed.hip), head width 32: the
// S^T = K Q^T / O^T += V^T P^T scheme in which a lane (g = lane / 16, n = lane % 16) holds eight scores of query n.
#pragma once
#include "evt_common.h"

namespace {

// two ds_read_b64_tr_b16 (transposing 16-bit LDS reads) -> one MFMA A fragment.  The builtin (not inline asm) lets the
// compiler track the LDS counter, so all fragment reads of a key sub-block are in flight behind ONE wait.
typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ h16x8 tr2(const h16_t* p0, const h16_t* p1) {
  typedef __attribute__((address_space(3))) s16x4* lds_p;
  union { struct { s16x4 lo, hi; } h; h16x8 v; } r;
  r.h.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p0));
  r.h.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p1));
  return r.v;
}

__device__ __forceinline__ h16x8 pack8(const float* p) {
  union { h16x8 v; h16_t e[8]; } r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.e[i] = f2h(p[i]);
  return r.v;
}

__device__ __forceinline__ h16x8 ld8(const h16_t* p) { return *reinterpret_cast<const h16x8*>(p); }

// k-slot e of lane group g inside a 32-wide block: e<4 -> g*4+e ; e>=4 -> 16 + g*4 + (e-4)
__device__ __forceinline__ int slot32(int g, int e) { return e < 4 ? g * 4 + e : 16 + g * 4 + (e - 4); }

}  // namespace

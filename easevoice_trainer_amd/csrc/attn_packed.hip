// Forward-only prefix-LM attention of the s1 prompt pass on a PACKED token axis, gfx950, with the layer's keys and values
// written into a stream session's cache by the same launch (auto_reg/t2s_infer.py T2SInfer._prompt_pass_packed).
// include/evt.h has the definition of the entry point (evt_attn_prefixlm_packed_fwd).
//
// Layout.  qkv [T][3 E], E = H * 32: sequence s owns rows tok0[s] .. tok0[s] + x_lens[s] + y_lens[s] - 1, its text rows
//   first, then its prompt rows; no padding.  The mask is attention.hip's `visible` without padded keys: inside a sequence
//   a text query (local index i < xl) sees the keys j < xl, an audio query the keys j <= i.  Nothing is read across a
//   sequence boundary: every row index is tok0[s] + (a local index below the sequence's own length).
// Work split.  The host lists the tiles (sequence, first local query), 64 queries each, counted from the sequence's OWN row
//   0: grid (tiles, H), no empty block, and a sequence's arithmetic does not depend on the pack around it.  A block has four
//   waves of 16 queries and walks the key tiles of 64 keys (two sub-blocks of 32) of its sequence in ascending order up to
//   kend = xl for a text tile, (its last live query) + 1 for a tile with audio queries; a wave skips the sub-blocks behind
//   its own 16 queries' bound.  Key tiles are double-buffered in LDS: tile t + 1 travels to registers while tile t is
//   multiplied and is written to the other buffer behind the arithmetic, one barrier per tile.  Rows at or behind kend are
//   zero-filled by ordinary writes and never read from memory.
// Arithmetic.  The transposed-score scheme of attention.hip / mha_rows.hip: S^T = K Q^T, so that lane (g = lane / 16,
//   n = lane % 16) holds the scores of query n against the keys slot32(g, e), e < 8, of a 32-key sub-block, the running
//   maximum of a query lives in its four lanes (two cross-lane steps), the running sum stays a per-lane partial until the
//   epilogue, and P^T is the B operand of O^T += V^T P^T without leaving the registers.  ONE tile walk (attn_packed_fwd) is
//   templated over the fragment loader:
//     FragH   16-bit input: mfma_f32_16x16x32 of the build's type, K rows by 16-byte LDS reads, V^T by ds_read_b64_tr_b16,
//             row pitch 40 elements (attention.hip's);
//     FragF   fp32 input: mfma_f32_16x16x4f32, true fp32 products, row pitch 36 floats, V by permuted 4-byte LDS reads
//             (mha_rows.hip's; q is multiplied once by scale * log2(e)).
//   Both leave channel 16 dt + 4 g + r of query n in register r of accumulator dt, so the epilogue is shared too.
// Cache write.  Block (tile, h) owns the K and V head rows of its 64 packed positions.  They are requested BEFORE the first
//   key tile and stored while that tile's loads are in flight, once per destination slot of the sequence (CSR row map:
//   dst_slot[dst_off[s] .. dst_off[s + 1])).  Local text position i -> cache position i, local audio position i ->
//   Xmax + (i - xl).  Slab caches [B][Lmax][E] take 16-byte pieces (converted when the cache dtype differs); the MXFP8
//   cache, head-major, takes the rows through mx_quant_row_store (mx8_quant.h), a wave-half per head row.  A slot outside
//   [0, B) or a position at or behind Lmax writes nothing.
// The descriptors are device memory the launcher cannot see: a tile whose sequence, lengths or rows fall outside [0, k) /
//   [0, T) makes its block return before any barrier, having read and written nothing.
#include "evt_common.h"
#include "attn_frag.h"
#include "mx8_quant.h"
#include "../../include/evt.h"
#include <type_traits>

namespace {

constexpr int PK_QT = EVT_ATTN_PACKED_QUERY_TILE, PK_KT = 64, PK_THREADS = 256;
static_assert(PK_QT == 64 && kD == 32, "four waves of 16 queries, head width 32");
enum { PK_SLAB_SAME = 0, PK_SLAB_OTHER = 1, PK_MX8 = 2 };

struct PkArgs {
  const void* qkv;
  void* out;
  const int *tok0, *x_lens, *y_lens, *tiles, *dst_off, *dst_slot;
  void *kc, *vc;          // slab [B][Lmax][E], or MXFP8 codes [B][H][Lmax][32]
  uint8_t *ks, *vs;       // MXFP8 scale bytes [B][H][Lmax]
  int T, k, n_dst, H, B, Lmax, Xmax;
  float c;                // scale * log2(e)
};

struct FragH {
  typedef h16_t T;
  static constexpr int P = kD + 8;
  struct Q { h16x8 v; };
  __device__ static Q load_q(const T* qrow, int g, float) {
    Q q;
    q.v = ld8(qrow + g * 8);
    return q;
  }
  __device__ static Q zero_q() {
    Q q;
#pragma unroll
    for (int i = 0; i < 8; ++i) q.v[i] = (evt_hn)0.f;
    return q;
  }
  __device__ static float post(float c) { return c; }      // the scores are raw: the walk multiplies them
  __device__ static void scores(const T* Kt, int n, int g, const Q& q, float* s) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 a = EVT_MFMA_16x16x32(ld8(Kt + n * P + g * 8), q.v, z, 0, 0, 0);
    const f32x4 b = EVT_MFMA_16x16x32(ld8(Kt + (16 + n) * P + g * 8), q.v, z, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) { s[r] = a[r]; s[4 + r] = b[r]; }
  }
  __device__ static void pv(const T* Vt, int n, int g, const float* p, f32x4* acc) {
    const T* vrow = Vt + (g * 4 + (n >> 2)) * P + 4 * (n & 3);
    const h16x8 va0 = tr2(vrow, vrow + 16 * P);
    const h16x8 va1 = tr2(vrow + 16, vrow + 16 * P + 16);
    const h16x8 pf = pack8(p);
    acc[0] = EVT_MFMA_16x16x32(va0, pf, acc[0], 0, 0, 0);
    acc[1] = EVT_MFMA_16x16x32(va1, pf, acc[1], 0, 0, 0);
  }
  __device__ static void store4(T* o, const float* v) {
    uint2 u;
    u.x = f2h_pack(v[0], v[1]);
    u.y = f2h_pack(v[2], v[3]);
    *reinterpret_cast<uint2*>(o) = u;
  }
};

struct FragF {
  typedef float T;
  static constexpr int P = kD + 4;
  struct Q { float v[2][4]; };
  __device__ static Q load_q(const T* qrow, int g, float c) {
    Q q;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const float4 z = *reinterpret_cast<const float4*>(qrow + 16 * cc + 4 * g);
      q.v[cc][0] = z.x * c; q.v[cc][1] = z.y * c; q.v[cc][2] = z.z * c; q.v[cc][3] = z.w * c;
    }
    return q;
  }
  __device__ static Q zero_q() {
    Q q;
#pragma unroll
    for (int i = 0; i < 8; ++i) q.v[i >> 2][i & 3] = 0.f;
    return q;
  }
  __device__ static float post(float) { return 1.f; }      // q carries scale * log2(e)
  __device__ static void scores(const T* Kt, int n, int g, const Q& q, float* s) {
    const T* kt = Kt + n * P + 4 * g;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const float4 kf = *reinterpret_cast<const float4*>(kt + st * 16 * P + 16 * cc);
        a = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.x, q.v[cc][0], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.y, q.v[cc][1], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.z, q.v[cc][2], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.w, q.v[cc][3], a, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) s[4 * st + r] = a[r];
    }
  }
  __device__ static void pv(const T* Vt, int n, int g, const float* p, f32x4* acc) {
    const T* vt = Vt + 4 * g * P + n;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vt[(st * 16 + r) * P + 16 * dt], p[4 * st + r], acc[dt], 0, 0, 0);
  }
  __device__ static void store4(T* o, const float* v) {
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
  }
};

// one 16-byte piece (segment sg) of a head row of T into the slab row `dst` (the head's first element) of CT
template <typename T, typename CT>
__device__ __forceinline__ void slab_store(CT* dst, int sg, const uint4& v) {
  if constexpr (std::is_same<T, CT>::value) {
    *reinterpret_cast<uint4*>(reinterpret_cast<char*>(dst) + sg * 16) = v;
  } else {
    constexpr int NE = 16 / (int)sizeof(T);
    union { uint4 u; T e[NE]; } r;
    r.u = v;
#pragma unroll
    for (int e = 0; e < NE; ++e) dst[sg * NE + e] = from_f<CT>(to_f<T>(r.e[e]));
  }
}

// grid (tiles, H), 256 threads
template <typename F, int CK>
__global__ __launch_bounds__(PK_THREADS) void attn_packed_fwd(PkArgs a) {
  typedef typename F::T T;
  typedef typename std::conditional<CK == PK_SLAB_SAME, T, typename std::conditional<std::is_same<T, float>::value, h16_t, float>::type>::type CT;
  constexpr int P = F::P, EP = 16 / (int)sizeof(T);            // row pitch; elements of a 16-byte piece
  constexpr int SEG = kD / EP, NL = PK_KT * SEG / PK_THREADS;   // pieces of a head row; pieces per thread, tile and operand
  constexpr int TILE = PK_KT * P;
  __shared__ __attribute__((aligned(16))) T Ks[2 * TILE];
  __shared__ __attribute__((aligned(16))) T Vs[2 * TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), n = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, E = a.H * kD;
  const int s = a.tiles[2 * blockIdx.x], q0 = a.tiles[2 * blockIdx.x + 1];
  if (s < 0 || s >= a.k) return;
  const int base = a.tok0[s], xl = a.x_lens[s], yl = a.y_lens[s];
  if (base < 0 || xl < 0 || yl < 0 || xl > a.T || yl > a.T) return;
  const int len = xl + yl;
  if (len > a.T - base || q0 < 0 || q0 >= len) return;         // all uniform over the block: no barrier is left waiting
  const T* rows = reinterpret_cast<const T*>(a.qkv) + (long)base * 3 * E + h * kD;      // q of local row 0, head h

  // ---- this block's own 64 positions: requested first, stored while key tile 0 is in flight ----
  int d0 = a.dst_off[s], d1 = a.dst_off[s + 1];
  d1 = d1 < a.n_dst ? d1 : a.n_dst;
  d0 = d0 < 0 ? d1 : d0;
  uint4 ok[NL], ov[NL];
  float mv[CK == PK_MX8 ? 16 : 1];
  if constexpr (CK == PK_MX8) {
    // item = 8 it + (wave-half): row = item / 2 of the tile, K or V = item % 2; the two halves of a wave share the row
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int item = it * 8 + (tid >> 5), i = q0 + (item >> 1);
      mv[it] = i < len ? to_f<T>(rows[(long)i * 3 * E + (1 + (item & 1)) * E + (tid & 31)]) : 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int idx = tid + j * PK_THREADS, i = q0 + idx / SEG, sg = idx % SEG;
      ok[j] = ov[j] = make_uint4(0, 0, 0, 0);
      if (i < len) {
        ok[j] = *reinterpret_cast<const uint4*>(rows + (long)i * 3 * E + E + sg * EP);
        ov[j] = *reinterpret_cast<const uint4*>(rows + (long)i * 3 * E + 2 * E + sg * EP);
      }
    }
  }

  const int qlast = min(q0 + PK_QT - 1, len - 1);
  const int kend = qlast < xl ? xl : qlast + 1;
  const int ntile = (kend + PK_KT - 1) / PK_KT;
  uint4 kr[NL], vr[NL];
  auto fetch = [&](int t) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int idx = tid + j * PK_THREADS, key = t * PK_KT + idx / SEG, sg = idx % SEG;
      kr[j] = vr[j] = make_uint4(0, 0, 0, 0);
      if (key < kend) {
        kr[j] = *reinterpret_cast<const uint4*>(rows + (long)key * 3 * E + E + sg * EP);
        vr[j] = *reinterpret_cast<const uint4*>(rows + (long)key * 3 * E + 2 * E + sg * EP);
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int idx = tid + j * PK_THREADS, row = idx / SEG, sg = idx % SEG;
      *reinterpret_cast<uint4*>(Ks + buf * TILE + row * P + sg * EP) = kr[j];
      *reinterpret_cast<uint4*>(Vs + buf * TILE + row * P + sg * EP) = vr[j];
    }
  };
  fetch(0);

  const int wq0 = q0 + wave * 16, qi = wq0 + n;                   // this lane's query
  const bool wlive = wq0 < len;
  const int wql = min(wq0 + 15, len - 1);
  const int wkend = wql < xl ? xl : wql + 1;                      // the wave's own key bound
  typename F::Q qf = F::zero_q();                                 // a dead query is not read: its column runs on zeros
  if (qi < len) qf = F::load_q(rows + (long)qi * 3 * E, g, a.c);

  // ---- the cache write ----
  if constexpr (CK == PK_MX8) {
    uint8_t* kq = reinterpret_cast<uint8_t*>(a.kc);
    uint8_t* vq = reinterpret_cast<uint8_t*>(a.vc);
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int item = it * 8 + (tid >> 5), i = q0 + (item >> 1), kv = item & 1;
      const int pos = i < xl ? i : a.Xmax + (i - xl);
      if (i >= len || pos >= a.Lmax || (i < xl && i >= a.Xmax)) continue;          // uniform over the wave
      for (int d = d0; d < d1; ++d) {
        const int slot = a.dst_slot[d];
        if (slot < 0 || slot >= a.B) continue;
        const long row = ((long)slot * a.H + h) * a.Lmax + pos;
        mx_quant_row_store(mv[it], tid & 31, (kv ? vq : kq) + row * kD, (kv ? a.vs : a.ks) + row);
      }
    }
  } else {
    CT* kc = reinterpret_cast<CT*>(a.kc);
    CT* vc = reinterpret_cast<CT*>(a.vc);
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int idx = tid + j * PK_THREADS, i = q0 + idx / SEG, sg = idx % SEG;
      const int pos = i < xl ? i : a.Xmax + (i - xl);
      if (i >= len || pos >= a.Lmax || (i < xl && i >= a.Xmax)) continue;
      for (int d = d0; d < d1; ++d) {
        const int slot = a.dst_slot[d];
        if (slot < 0 || slot >= a.B) continue;
        const long row = ((long)slot * a.Lmax + pos) * E + h * kD;
        slab_store<T, CT>(kc + row, sg, ok[j]);
        slab_store<T, CT>(vc + row, sg, ov[j]);
      }
    }
  }

  stash(0);
  __syncthreads();

  const float cp = F::post(a.c);
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  float mrun = -INFINITY, lrun = 0.f;                             // the query's running max; this lane's share of the sum
  for (int t = 0; t < ntile; ++t) {
    if (t + 1 < ntile) fetch(t + 1);
    if (wlive) {
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
        const int k0 = t * PK_KT + sb * 32;
        if (k0 >= wkend) continue;                                // wave-uniform: behind every query of the wave
        float sc[8];
        F::scores(Ks + (t & 1) * TILE + sb * 32 * P, n, g, qf, sc);
        float mt = -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int kj = k0 + slot32(g, e);
          const bool vis = qi < xl ? kj < xl : kj <= qi;
          sc[e] = vis ? sc[e] * cp : -INFINITY;
          mt = fmaxf(mt, sc[e]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float mnew = fmaxf(mrun, mt);
        const float ms = mnew == -INFINITY ? 0.f : mnew;          // nothing visible yet: every exp2 below gives 0
        const float alpha = __builtin_amdgcn_exp2f(mrun - ms);
        mrun = mnew;
        float psum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          sc[e] = __builtin_amdgcn_exp2f(sc[e] - ms);
          psum += sc[e];
        }
        lrun = lrun * alpha + psum;
        acc[0] *= alpha;
        acc[1] *= alpha;
        F::pv(Vs + (t & 1) * TILE + sb * 32 * P, n, g, sc, acc);
      }
    }
    if (t + 1 < ntile) stash((t + 1) & 1);                        // that buffer was last read before the previous barrier
    __syncthreads();
  }

  lrun += __shfl_xor(lrun, 16, 64);                               // (l_g + l_g^1) + (l_g^2 + l_g^3): the same bits in all four lanes
  lrun += __shfl_xor(lrun, 32, 64);
  if (qi >= len) return;
  const float inv = lrun > 0.f ? 1.f / lrun : 0.f;
  T* orow = reinterpret_cast<T*>(a.out) + (long)(base + qi) * E + h * kD + 4 * g;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    const float o4[4] = {acc[dt][0] * inv, acc[dt][1] * inv, acc[dt][2] * inv, acc[dt][3] * inv};
    F::store4(orow + 16 * dt, o4);
  }
}

template <typename F>
int pk_launch(const PkArgs& a, int ck, int nt, hipStream_t st) {
  const dim3 grid(nt, a.H), block(PK_THREADS);
  if (ck == PK_SLAB_SAME) hipLaunchKernelGGL((attn_packed_fwd<F, PK_SLAB_SAME>), grid, block, 0, st, a);
  else if (ck == PK_SLAB_OTHER) hipLaunchKernelGGL((attn_packed_fwd<F, PK_SLAB_OTHER>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((attn_packed_fwd<F, PK_MX8>), grid, block, 0, st, a);
  return evt_check_launch();
}

}  // namespace

extern "C" int evt_attn_prefixlm_packed_fwd(int32_t dtype, const void* qkv, void* out, const int32_t* tok0,
                                            const int32_t* x_lens, const int32_t* y_lens, const int32_t* tiles,
                                            const int32_t* dst_off, const int32_t* dst_slot, int32_t cache_fmt,
                                            int32_t cdtype, void* kcache, void* vcache, uint8_t* kscales, uint8_t* vscales,
                                            int32_t T, int32_t k, int32_t nt, int32_t n_dst, int32_t H, int32_t D, int32_t B,
                                            int32_t Lmax, int32_t Xmax, void* stream) {
  if (!qkv || !out || !tok0 || !x_lens || !y_lens || !tiles || !dst_off || !dst_slot || !kcache || !vcache) return EVT_EINVAL;
  if (T <= 0 || k <= 0 || nt <= 0 || n_dst < 0 || H <= 0 || H > 65535 || B <= 0 || Lmax <= 0 || Xmax < 0) return EVT_EINVAL;
  if (dtype != EVT_DT_F32 && dtype != EVT_DT_HALF) return EVT_EINVAL;
  int ck;
  if (cache_fmt == EVT_KV_FMT_MX8) {
    if (!kscales || !vscales) return EVT_EINVAL;
    ck = PK_MX8;
  } else if (cache_fmt == EVT_KV_FMT_SLAB) {
    if (cdtype != EVT_DT_F32 && cdtype != EVT_DT_HALF) return EVT_EINVAL;
    ck = cdtype == dtype ? PK_SLAB_SAME : PK_SLAB_OTHER;
  } else {
    return EVT_EINVAL;
  }
  if (D != kD) return EVT_ENOTSUP;
  if (((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)kcache | (uintptr_t)vcache) & 15) return EVT_EINVAL;
  PkArgs a{qkv, out, tok0, x_lens, y_lens, tiles, dst_off, dst_slot, kcache, vcache, kscales, vscales,
           T, k, n_dst, H, B, Lmax, Xmax, 1.44269504088896340736f / sqrtf((float)kD)};
  if (dtype == EVT_DT_F32) return pk_launch<FragF>(a, ck, nt, (hipStream_t)stream);
  return pk_launch<FragH>(a, ck, nt, (hipStream_t)stream);
}

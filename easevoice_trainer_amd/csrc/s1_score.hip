// Teacher-forced scoring head of the s1 model for gfx950: logits of many positions at once and, per position, the two
// log-probabilities evt_dec_sample_embed_rows_f reports for a forced step (auto_reg/t2s_infer.py score_stream with
// prompt_pass="teacher").  include/evt.h has the definition of the entry point (evt_score_rows).
//
// Work split.  One workgroup of 16 waves per tile of 16 scored positions of ONE sequence, counted from the sequence's own
//   index 0, so a sequence's arithmetic does not depend on the launch around it.  Two phases, one barrier apart:
//   logits   the 16 x E tile of h is staged once in LDS (rows behind the sequence's last index are zero); Wp is streamed
//            from memory in column tiles of 16, tile c to wave c % 16; D[column][position] comes out of the MFMA with the
//            column on (lane >> 4) * 4 + reg and the position on lane & 15 and goes to LDS as fp32, never to memory.
//              fp32    mfma_f32_16x16x4f32, lane group g owning 16 consecutive k of every 64 (s1_decode_rows.hip's
//                      scheme: exact fp32 products, two accumulation chains);
//              16-bit  mfma_f32_16x16x32 of the build's type on 16-byte fragments (attn_frag.h's ld8), lane group g
//                      owning 8 consecutive k of every 32.
//            Rows of Wp at or behind V are fed as zeros and their columns are not stored (the masked last tile).  When
//            h tile + logits would not fit the LDS (E = 1024 next to V = 2048), K is walked in chunks: the tile of h is
//            restaged per chunk and a lane adds to the logits it stored itself.
//   finish   wave w finishes position w on its own: no workgroup-wide sort, no barrier.  A lane keeps the logits
//            v = lane + 64 u in registers (NV = 17 or 32 of them).
// Seen tokens.  The repetition penalty needs the set of tokens before a position.  The tile's common part -- the history
//   before its first position -- is one bitmap of 2048 bits built by all threads with LDS atomics while the first weights
//   travel; position w's view is that bitmap plus the w tokens between the tile's start and itself, one word per lane.
// Selection in place of the sort.  Only the score of ONE column is wanted, and both cuts of the sampler keep a prefix of
//   the sorted order (descending value, ascending index among equals), so the kernel looks for the two boundaries, not
//   for the order:
//     nucleus  entry at rank r goes when r > 0 and cum(r) > top_p.  cum of the LAST entry of a value t is
//              S(t) = sum(e_v : x_v >= t) / total, a masked sum in a fixed lane order and therefore monotone in t: a
//              bitwise search over the 32 bits of the ordered key finds t* = the largest value with S(t*) > top_p, the
//              value the cut falls into; inside it, entries are equal, and the j-th goes when
//              sum(e_v : x_v > t*) + (j + 1) e_t* exceeds top_p * total -- counted up, first index first.
//     top-k    the k-th largest value by the same search on counts (ballots); the k-th ENTRY is the
//              (k - 1 - #{x > x_k})-th among its equals, which says whether the nucleus took it (then there is no
//              pivot, as cur[si[k - 1]] = -inf in sample_row); otherwise every value with x / T >= x_k / T stays.
//   The decisions are those of the sorted form, ties included; 2 x 32 wave reductions replace a 2048-wide bitonic sort.
// LDS (dynamic): logits 16 x (16 ceil(V / 16) + 1) fp32 (66.6 KB at V = 1025), h tile 16 x (chunk + pad) in dtype (33 KB
//   fp32 / 16.6 KB 16-bit at E = 512), bitmaps 17 x 256 B: 104 KB at the model's shape in fp32, one workgroup per CU.
//   The launcher picks the largest K chunk out of E, 512, 256, 128, 64 that keeps the total under 160 KB.
// The descriptors are device memory the launcher cannot see: a tile with anything out of range returns before its first
//   barrier, having read nothing but descriptors and written nothing.
#include "evt_common.h"
#include "attn_frag.h"
#include "../../include/evt.h"

namespace {

constexpr int SC_TILE = EVT_SCORE_ROWS_TILE, SC_THREADS = 1024, SC_WAVES = 16, SC_BM = 64;   // bitmap words: 2048 bits
static_assert(SC_TILE == 16 && SC_WAVES == SC_TILE, "one wave per position, one MFMA tile of positions");

struct ScArgs {
  const void *h, *Wp;
  const int *hist, *hist0, *row0, *P, *f, *tiles;
  const evt_row_sample* rs;
  float* logp;
  int no_eos_steps, k, T, E, V, n_hist, n_out, KC;
};

template <typename T> struct ScK;
template <> struct ScK<float> { static constexpr int SL = 64, PAD = 4; };     // K slice of an MFMA round, LDS row pad
template <> struct ScK<h16_t> { static constexpr int SL = 32, PAD = 8; };

__host__ __device__ constexpr int sc_up(int v, int m) { return (v + m - 1) / m * m; }
template <typename T> __host__ __device__ constexpr int sc_hs(int kc) { return sc_up(kc, ScK<T>::SL) + ScK<T>::PAD; }
__host__ __device__ constexpr int sc_vs(int V) { return sc_up(V, 16) + 1; }
template <typename T> size_t sc_lds(int V, int kc) {
  return (size_t)SC_TILE * sc_vs(V) * 4 + (size_t)sc_up(SC_TILE * sc_hs<T>(kc) * (int)sizeof(T), 16) + (SC_WAVES + 1) * SC_BM * 4;
}

// one column tile of one K chunk: acc[r] = sum_k Wp[n0 + 4 g + r][k0 + k] * h[j][k0 + k], j = lane & 15, g = lane >> 4
__device__ __forceinline__ f32x4 sc_tile(const float* wrow, bool live, const float* hs, int HS, int kc, int j, int g) {
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
  for (int ks = 0; ks < kc; ks += 64) {
    const int kk = ks + 16 * g;
    float wf[16], xv[16];
    const bool on = live && kk < kc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 w4 = on ? *reinterpret_cast<const float4*>(wrow + kk + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 x4 = *reinterpret_cast<const float4*>(hs + j * HS + kk + 4 * q);
      wf[4 * q] = w4.x; wf[4 * q + 1] = w4.y; wf[4 * q + 2] = w4.z; wf[4 * q + 3] = w4.w;
      xv[4 * q] = x4.x; xv[4 * q + 1] = x4.y; xv[4 * q + 2] = x4.z; xv[4 * q + 3] = x4.w;
    }
#pragma unroll
    for (int e = 0; e < 16; e += 2) {
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[e], xv[e], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[e + 1], xv[e + 1], a1, 0, 0, 0);
    }
  }
  return a0 + a1;
}

__device__ __forceinline__ f32x4 sc_tile(const h16_t* wrow, bool live, const h16_t* hs, int HS, int kc, int j, int g) {
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
  h16x8 z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = (evt_hn)0.f;
  for (int ks = 0; ks < kc; ks += 64) {
    const int k0 = ks + 8 * g, k1 = k0 + 32;
    const h16x8 w0 = live && k0 < kc ? ld8(wrow + k0) : z;
    const h16x8 w1 = live && k1 < kc ? ld8(wrow + k1) : z;
    a0 = EVT_MFMA_16x16x32(w0, ld8(hs + j * HS + k0), a0, 0, 0, 0);
    if (ks + 32 < kc) a1 = EVT_MFMA_16x16x32(w1, ld8(hs + j * HS + k1), a1, 0, 0, 0);
  }
  return a0 + a1;
}

// ordered key <-> float: key order is float order; keys below -inf's read as -inf, keys above +inf's are NaN (never >=)
__device__ __forceinline__ float sc_unkey(unsigned k) {
  if (k < 0x007fffffu) k = 0x007fffffu;
  return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k);
}

__device__ __forceinline__ int wave_count(bool c) { return __popcll(__ballot(c)); }

// Position `w` of the tile, by one wave.  lg: its V logits in LDS; bm: its seen-token bitmap; tok: the given token; Ve:
// the columns of its step.  x[] holds NaN in the slots at or behind Ve: no comparison takes them, fmaxf drops them.
template <int NV>
__device__ __forceinline__ void sc_finish(const float* lg, const unsigned* bm, int V, int Ve, int tok,
                                          const evt_row_sample r, float* out) {
  const int lane = threadIdx.x & 63;
  float x[NV], e[NV];
  // ---- [0]: log_softmax of the raw logits ----
  float rmax = -INFINITY;
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int v = lane + 64 * u;
    x[u] = v < Ve ? lg[v] : NAN;
    rmax = fmaxf(rmax, x[u]);
  }
  rmax = wave_reduce_max(rmax);
  float rsum = 0.f;
#pragma unroll
  for (int u = 0; u < NV; ++u)
    if (lane + 64 * u < Ve) rsum += expf(x[u] - rmax);
  rsum = wave_reduce_sum(rsum);
  const bool tok_ok = (unsigned)tok < (unsigned)V;
  const float o0 = !tok_ok ? NAN : tok >= Ve ? -INFINITY : lg[tok] - rmax - logf(rsum);
  // ---- repetition penalty, then e = exp(x - max) of the penalised logits ----
  float m = -INFINITY;
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int v = lane + 64 * u;
    if (r.repetition_penalty != 1.0f && v < Ve && ((bm[v >> 5] >> (v & 31)) & 1u))
      x[u] = x[u] < 0.f ? x[u] * r.repetition_penalty : x[u] / r.repetition_penalty;
    m = fmaxf(m, x[u]);
  }
  m = wave_reduce_max(m);
  // ---- nucleus boundary (t*, jstar): entries above t* stay, of those equal to t* the first jstar ----
  float tstar = -INFINITY;
  int jstar = 0x7fffffff;
  if (r.top_p < 1.0f) {
    float total = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      e[u] = lane + 64 * u < Ve ? expf(x[u] - m) : 0.f;
      total += e[u];
    }
    total = wave_reduce_sum(total);
    unsigned key = 0;
    for (int b = 31; b >= 0; --b) {
      const float t = sc_unkey(key | (1u << b));
      float s = 0.f;
#pragma unroll
      for (int u = 0; u < NV; ++u) s += x[u] >= t ? e[u] : 0.f;
      s = wave_reduce_sum(s);
      if (s / total > r.top_p) key |= 1u << b;
    }
    tstar = sc_unkey(key);
    if (!(tstar <= m)) tstar = m;                 // top_p < 0 (or NaN logits): the cut falls into the first value
    float sgt = 0.f;
    int nt = 0;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      sgt += x[u] > tstar ? e[u] : 0.f;
      nt += wave_count(x[u] == tstar);
    }
    float c = wave_reduce_sum(sgt);
    const float et = expf(tstar - m);
    for (jstar = 0; jstar < nt; ++jstar) {
      c += et;
      if (c / total > r.top_p) break;
    }
    if (jstar == 0 && tstar == m) jstar = 1;      // the first sorted entry is always kept
  }
  // ---- top-k pivot ----
  const float tdiv = fmaxf(r.temperature, 1e-5f);
  float pivot = -INFINITY;
  if (r.top_k > 0) {
    const int kk = r.top_k < Ve ? r.top_k : Ve;
    unsigned key = 0;
    for (int b = 31; b >= 0; --b) {
      const float t = sc_unkey(key | (1u << b));
      int n = 0;
#pragma unroll
      for (int u = 0; u < NV; ++u) n += wave_count(x[u] >= t);
      if (n >= kk) key |= 1u << b;
    }
    const float xk = sc_unkey(key);
    int ngt = 0;
#pragma unroll
    for (int u = 0; u < NV; ++u) ngt += wave_count(x[u] > xk);
    if (xk > tstar || (xk == tstar && kk - 1 - ngt < jstar)) pivot = xk / tdiv;
  }
  // ---- softmax over the survivors, read at the token ----
  const float mx = m / tdiv;
  float sum = 0.f, mine = -INFINITY;
  int seen_eq = 0;                                  // entries equal to t* in the slots before u
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const bool eq = x[u] == tstar;
    const unsigned long long bal = __ballot(eq);
    const int tie = seen_eq + __popcll(bal & ((1ull << lane) - 1ull));
    seen_eq += __popcll(bal);
    const float y = x[u] / tdiv;
    const bool keep = (x[u] > tstar || (eq && tie < jstar)) && y >= pivot;
    const float d = keep ? y - mx : -INFINITY;
    sum += keep ? expf(d) : 0.f;
    if (lane + 64 * u == tok) mine = d;
  }
  sum = wave_reduce_sum(sum);
  mine = wave_reduce_max(mine);
  if (lane == 0) {
    out[0] = o0;
    out[1] = !tok_ok ? NAN : mine - logf(sum);
  }
}

template <typename T>
__global__ __launch_bounds__(SC_THREADS) void score_rows(const ScArgs a) {
  extern __shared__ __align__(16) unsigned char sc_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int E = a.E, V = a.V, VS = sc_vs(V), HS = sc_hs<T>(a.KC);
  float* lgs = reinterpret_cast<float*>(sc_smem);                                  // [16][VS]
  T* hs = reinterpret_cast<T*>(sc_smem + (size_t)SC_TILE * VS * 4);                // [16][HS]
  unsigned* base = reinterpret_cast<unsigned*>(sc_smem + (size_t)SC_TILE * VS * 4 + sc_up(SC_TILE * HS * (int)sizeof(T), 16));
  unsigned* bms = base + SC_BM;                                                    // [16][SC_BM]
  // ---- descriptors: all uniform over the workgroup, every return is taken by all threads before the first barrier ----
  const int s = a.tiles[2 * blockIdx.x], q0 = a.tiles[2 * blockIdx.x + 1];
  if (s < 0 || s >= a.k) return;
  const int P = a.P[s], f = a.f[s], h0 = a.hist0[s], r0 = a.row0[s];
  if (P < 0 || f <= 0 || q0 < 0 || q0 >= f || (q0 & (SC_TILE - 1))) return;
  if (h0 < 0 || (long)h0 + P + f > a.n_hist || r0 < 0 || (long)r0 + f > a.T) return;
  long out0 = 0;
  for (int t = 0; t < s; ++t) {
    const int ft = a.f[t];
    if (ft < 0) return;
    out0 += ft;
  }
  if (out0 + f > a.n_out) return;
  const int npos = f - q0 < SC_TILE ? f - q0 : SC_TILE;       // live positions of the tile
  const evt_row_sample rs = a.rs[s];

  if (tid < SC_BM) base[tid] = 0u;
  const T* hg = reinterpret_cast<const T*>(a.h) + (long)(r0 + q0) * E;
  const T* Wp = reinterpret_cast<const T*>(a.Wp);
  constexpr int PV = 16 / (int)sizeof(T);                     // elements of a 16-byte piece
  const int nct = (V + 15) / 16;
  for (int k0 = 0; k0 < E; k0 += a.KC) {
    const int kc = E - k0 < a.KC ? E - k0 : a.KC;
    if (k0 > 0) __syncthreads();                              // every wave is done with the previous chunk of h
    const int ppr = (HS - ScK<T>::PAD) / PV;                  // pieces per row, the zero tail of the last slice included
    for (int i = tid; i < SC_TILE * ppr; i += SC_THREADS) {
      const int row = i / ppr, c = (i % ppr) * PV;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (row < npos && c < kc) v = *reinterpret_cast<const uint4*>(hg + (long)row * E + k0 + c);
      *reinterpret_cast<uint4*>(hs + row * HS + c) = v;
    }
    __syncthreads();
    if (k0 == 0)                                              // the tile's common history: behind the barrier that zeroed it
      for (int i = tid; i < P + q0; i += SC_THREADS) {
        const int t = a.hist[h0 + i];
        if (t >= 0 && t < V) atomicOr(&base[t >> 5], 1u << (t & 31));
      }
    for (int ct = wave; ct < nct; ct += SC_WAVES) {
      const int n = ct * 16 + j;
      const f32x4 acc = sc_tile(Wp + (long)(n < V ? n : 0) * E + k0, n < V, hs, HS, kc, j, g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int v = ct * 16 + 4 * g + r;
        if (v < V) {
          float* o = lgs + j * VS + v;
          *o = k0 == 0 ? acc[r] : *o + acc[r];
        }
      }
    }
  }
  __syncthreads();                                            // logits and the common bitmap are complete
  {
    unsigned word = base[lane];
    for (int t = 0; t < wave && t < npos; ++t) {              // the tokens between the tile's start and this position
      const int tk = a.hist[h0 + P + q0 + t];
      if (tk >= 0 && tk < V && (tk >> 5) == lane) word |= 1u << (tk & 31);
    }
    bms[wave * SC_BM + lane] = word;
  }
  __syncthreads();
  if (wave >= npos) return;
  const int i = q0 + wave;
  const int Ve = i < a.no_eos_steps ? V - 1 : V;
  const int tok = a.hist[h0 + P + i];
  float* out = a.logp + (out0 + i) * 2;
  if (V <= 17 * 64) sc_finish<17>(lgs + wave * VS, bms + wave * SC_BM, V, Ve, tok, rs, out);
  else sc_finish<32>(lgs + wave * VS, bms + wave * SC_BM, V, Ve, tok, rs, out);
}

template <typename T>
int sc_launch(ScArgs a, int nt, hipStream_t st) {
  static size_t lds_set = 0;         // more than 64 KB of dynamic LDS needs the attribute; raised as shapes ask for it
  a.KC = 0;
  for (int kc : {a.E, 512, 256, 128, 64})
    if (kc <= a.E && sc_lds<T>(a.V, kc) <= 160 * 1024) { a.KC = kc; break; }
  if (a.KC == 0) return EVT_ENOTSUP;
  const size_t lds = sc_lds<T>(a.V, a.KC);
  if (lds > lds_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&score_rows<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
      return EVT_ELAUNCH;
    lds_set = lds;
  }
  hipLaunchKernelGGL(score_rows<T>, dim3(nt), dim3(SC_THREADS), lds, st, a);
  return evt_check_launch();
}

}  // namespace

extern "C" int evt_score_rows(int32_t dtype, const void* h, const void* Wp, const int32_t* hist, const int32_t* hist0,
                              const int32_t* row0, const int32_t* P, const int32_t* f, const evt_row_sample* row_sample,
                              const int32_t* tiles, float* logp, int32_t eos, int32_t no_eos_steps, int32_t k, int32_t nt,
                              int32_t T, int32_t E, int32_t V, int32_t n_hist, int32_t n_out, void* stream) {
  if (!h || !Wp || !hist || !hist0 || !row0 || !P || !f || !row_sample || !tiles || !logp) return EVT_EINVAL;
  if (k <= 0 || nt <= 0 || T <= 0 || n_hist <= 0 || n_out <= 0) return EVT_EINVAL;
  if (dtype != EVT_DT_F32 && dtype != EVT_DT_BF16 && dtype != EVT_DT_F16) return EVT_EINVAL;
  if ((((uintptr_t)h | (uintptr_t)Wp) & 15) || ((uintptr_t)logp & 3)) return EVT_EINVAL;
  if (E <= 0 || E % 16 || E > 1024 || V < 2 || V > 2048) return EVT_ENOTSUP;
  if (dtype != EVT_DT_F32 && dtype != EVT_DT_HALF) return EVT_ENOTSUP;
  if (eos != V - 1) return EVT_EINVAL;
  ScArgs a{h, Wp, hist, hist0, row0, P, f, tiles, row_sample, logp, no_eos_steps, k, T, E, V, n_hist, n_out, 0};
  if (dtype == EVT_DT_F32) return sc_launch<float>(a, nt, (hipStream_t)stream);
  return sc_launch<h16_t>(a, nt, (hipStream_t)stream);
}

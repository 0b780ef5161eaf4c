// Device code shared by the s1 decode kernels (s1_decode.hip: sessions with one set of counters; s1_decode_stream.hip:
// per-row counters): block reductions, the cache-attention body and the sampler body.  Everything lives in an anonymous
// namespace, so each translation unit gets its own copy.
#pragma once
#include "evt_common.h"
#include "../../include/evt.h"

namespace {

__device__ __forceinline__ float block_sum(float v, float* red, int nwaves) {
  v = wave_reduce_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < nwaves; ++i) s += red[i];
  return s;
}

__device__ __forceinline__ float block_max(float v, float* red, int nwaves) {
  v = wave_reduce_max(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = -INFINITY;
  for (int i = 0; i < nwaves; ++i) s = fmaxf(s, red[i]);
  return s;
}

// (value, index) argmax with the FIRST index among equal values (torch.argmax on CPU); all threads get the result
__device__ __forceinline__ int block_argmax(float v, int i, float* redv, int* redi, int nwaves) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) { redv[w] = v; redi[w] = i; }
  __syncthreads();
  float bv = redv[0];
  int bi = redi[0];
  for (int k = 1; k < nwaves; ++k)
    if (redv[k] > bv || (redv[k] == bv && redi[k] < bi)) { bv = redv[k]; bi = redi[k]; }
  return bi;
}

template <typename T> struct WVec { static constexpr int V = 16 / sizeof(T); };

// ---- append (k, v) of the new token to the cache, attend over all cached positions -------------------------------
// Scores: one key per thread (D elements = D/V 16-byte loads, all in flight).  P.V: a thread owns one 16-byte chunk of
// the value rows of every G-th key (G = 256 / chunks-per-row), so the cache is read with 16-byte loads only; the G
// partial rows are summed through LDS.  The first key row and the first PF value chunks of a thread depend on nothing
// computed in the launch and are requested before anything else (Prefetch), the rest follows the softmax.
template <typename T, int D> struct AttnShape {
  static constexpr int V = WVec<T>::V;
  static constexpr int C = D / V;        // 16-byte chunks per row
  static constexpr int G = 256 / C;      // key groups in the P.V phase
  static constexpr int PF = 8;
};

template <typename T, int D> struct Prefetch {
  uint4 u0[AttnShape<T, D>::C], vpre[AttnShape<T, D>::PF];
  __device__ __forceinline__ void issue(const T* kc, const T* vc, int b, int h, int E, int Lmax, int L, int pos) {
    using S = AttnShape<T, D>;
    const int tid = threadIdx.x, g = tid / S::C, c = tid % S::C;
    if (tid < L && tid != pos) {
      const T* row = kc + ((long)b * Lmax + tid) * E + h * D;
#pragma unroll
      for (int cc = 0; cc < S::C; ++cc) u0[cc] = *reinterpret_cast<const uint4*>(row + cc * S::V);
    }
#pragma unroll
    for (int i = 0; i < S::PF; ++i) {
      const int j = g + i * S::G;
      if (j < L && j != pos) vpre[i] = *reinterpret_cast<const uint4*>(vc + ((long)b * Lmax + j) * E + h * D + c * S::V);
    }
  }
};

// qs (scaled query), kn / vn (new key / value, already rounded to the cache dtype) are in LDS and published
template <typename T, int D>
__device__ __forceinline__ void attn_tail(const Prefetch<T, D>& pf, const float* qs, const float* kn, const float* vn,
                                          float* sc, float* red, float (*part)[D + 1], const T* kc, const T* vc,
                                          float* __restrict__ out, int b, int h, int E, int Lmax, int L, int pos,
                                          int mlo, int mhi) {
  // keys mlo <= j < mhi are padding of a shorter text in a batch (infer_panel_batch_infer's padding mask): skipped
  using S = AttnShape<T, D>;
  constexpr int V = S::V, C = S::C, G = S::G, PF = S::PF;
  const int tid = threadIdx.x, g = tid / C, c = tid % C;
  float mx = -INFINITY;
  for (int j = tid; j < L; j += 256) {
    float s = 0.f;
    if (j >= mlo && j < mhi) {
      s = -INFINITY;
    } else if (j == pos) {
#pragma unroll
      for (int d = 0; d < D; ++d) s += qs[d] * kn[d];
    } else {
      uint4 u[C];
      if (j == tid) {
#pragma unroll
        for (int cc = 0; cc < C; ++cc) u[cc] = pf.u0[cc];
      } else {
        const T* row = kc + ((long)b * Lmax + j) * E + h * D;
#pragma unroll
        for (int cc = 0; cc < C; ++cc) u[cc] = *reinterpret_cast<const uint4*>(row + cc * V);
      }
#pragma unroll
      for (int cc = 0; cc < C; ++cc) {
        const T* pu = reinterpret_cast<const T*>(&u[cc]);
#pragma unroll
        for (int e = 0; e < V; ++e) s += qs[cc * V + e] * to_f<T>(pu[e]);
      }
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
  float acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = 0.f;
#pragma unroll
  for (int i = 0; i < PF; ++i) {
    const int j = g + i * G;
    if (j < L) {
      const float pj = sc[j];
      if (j == pos) {
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += pj * vn[c * V + e];
      } else {
        const T* pu = reinterpret_cast<const T*>(&pf.vpre[i]);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += pj * to_f<T>(pu[e]);
      }
    }
  }
  for (int j = g + PF * G; j < L; j += G) {
    const float pj = sc[j];
    if (j == pos) {
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] += pj * vn[c * V + e];
    } else {
      const uint4 u = *reinterpret_cast<const uint4*>(vc + ((long)b * Lmax + j) * E + h * D + c * V);
      const T* pu = reinterpret_cast<const T*>(&u);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] += pj * to_f<T>(pu[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) part[g][c * V + e] = acc[e];
  __syncthreads();
  if (tid < D) {
    float o = 0.f;
#pragma unroll 8
    for (int i = 0; i < G; ++i) o += part[i][tid];
    out[(long)b * E + h * D + tid] = o / sum;
  }
}

__device__ __forceinline__ unsigned mix32s(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

__device__ __forceinline__ bool before(float av, int ai, float bv, int bi) {   // descending value, ascending index
  return av > bv || (av == bv && ai < bi);
}

constexpr int kSortN = 2048;

// ---- sample() of one row: repetition penalty, bitonic sort, nucleus / top-k pivots, temperature, argmax(p / q) ------
// Called by all 1024 threads of a workgroup.  lg: the row's logits; yb[0..ycount): its tokens so far; q_row: the V noise
// values of this (step, row) from an injected table, or NULL for the built-in noise keyed by (nseed, idx, nlane, v).
// Returns the token on every thread; *amax is the arg-max of the penalised logits (the EOS test of t2s_model.py:846).
// kLp (dec_sample_embed_rows_lp only): the thread that owns the token also stores log(pr[token]) to *slp (LDS), as
// x - max - log(sum) of the values pr is the softmax of, so a surviving token never underflows to -inf; the caller reads
// it after a barrier.  With kLp = false the function is the one every other sampler kernel has always compiled.
// kForce (dec_sample_embed_rows_f only): `ftok` >= 0 is a token GIVEN for this step (the same value on every thread of
// the workgroup); the draw runs as ever and is returned, but the log-probability stored to *slp is that of column ftok,
// reported by the thread that owns the column whether or not it won the arg-max: -inf when the sampler had cut it.
// ftok < 0 (no given token) and kForce = false leave every instruction as it was.
template <bool kLp = false, bool kForce = false>
__device__ __forceinline__ int sample_row(const evt_sample_params& p, const float* __restrict__ lg, const long* yb,
                                          int idx, int ycount, unsigned nseed, unsigned nlane,
                                          const float* __restrict__ q_row, float* probs_row, int* amax_out,
                                          float* slp = nullptr, int ftok = -1) {
  __shared__ float sv[kSortN];
  __shared__ int si[kSortN];
  __shared__ float cur[kSortN];
  __shared__ unsigned char flag[kSortN];
  __shared__ float redv[16];
  __shared__ int redi[16];
  __shared__ float wsum[16];
  const int tid = threadIdx.x, V = p.V;
  const int Ve = idx < p.no_eos_steps ? V - 1 : V;     // "at least 10 tokens otherwise not stop", t2s_model.py:833
  for (int v = tid; v < kSortN; v += 1024) flag[v] = 0;
  __syncthreads();
  if (p.repetition_penalty != 1.0f)
    for (int j = tid; j < ycount; j += 1024) {
      const long t = yb[j];
      if (t >= 0 && t < Ve) flag[t] = 1;
    }
  __syncthreads();
  float bvv = -INFINITY;
  int bii = 0x7fffffff;
  for (int v = tid; v < kSortN; v += 1024) {
    float x = -INFINITY;
    if (v < Ve) {
      x = lg[v];
      if (flag[v]) x = x < 0.f ? x * p.repetition_penalty : x / p.repetition_penalty;
      if (x > bvv || (x == bvv && v < bii)) { bvv = x; bii = v; }
    }
    cur[v] = x;
    sv[v] = x;
    si[v] = v;
  }
  // argmax of the (penalised, in place in the reference) logits: the EOS test of t2s_model.py:846
  const int amax = block_argmax(bvv, bii, redv, redi, 16);
  // bitonic sort, descending
  for (int k = 2; k <= kSortN; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      const int i = 2 * j * (tid / j) + (tid % j), l = i + j;
      const bool up = (i & k) == 0;
      const float av = sv[i], bv = sv[l];
      const int ai = si[i], bi = si[l];
      const bool in_order = before(av, ai, bv, bi);
      if (in_order != up) { sv[i] = bv; sv[l] = av; si[i] = bi; si[l] = ai; }
    }
  __syncthreads();
  if (p.top_p < 1.0f) {
    // cumulative softmax over the sorted logits; entries past the nucleus are removed, the first is always kept
    const float m = sv[0];
    const float e0 = expf(sv[2 * tid] - m), e1 = expf(sv[2 * tid + 1] - m);
    float run = e0 + e1;
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float t = __shfl_up(run, o, 64);
      if (lane >= o) run += t;
    }
    if (lane == 63) wsum[w] = run;
    __syncthreads();
    float offs = 0.f, total = 0.f;
    for (int i = 0; i < 16; ++i) {
      if (i < w) offs += wsum[i];
      total += wsum[i];
    }
    const float c1 = (offs + run) / total, c0 = (offs + run - e1) / total;
    if (2 * tid > 0 && c0 > p.top_p && si[2 * tid] < Ve) cur[si[2 * tid]] = -INFINITY;
    if (c1 > p.top_p && si[2 * tid + 1] < Ve) cur[si[2 * tid + 1]] = -INFINITY;
    __syncthreads();
  }
  const float tdiv = fmaxf(p.temperature, 1e-5f);
  float pivot = -INFINITY;
  if (p.top_k > 0) {
    const int kk = p.top_k < Ve ? p.top_k : Ve;
    pivot = cur[si[kk - 1]] / tdiv;
  }
  float x0[2], mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int v = tid + u * 1024;
    float x = -INFINITY;
    if (v < Ve) {
      x = cur[v] / tdiv;
      if (x < pivot) x = -INFINITY;
    }
    x0[u] = x;
    mx = fmaxf(mx, x);
  }
  mx = block_max(mx, redv, 16);
  float e[2], sum = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    e[u] = x0[u] == -INFINITY ? 0.f : expf(x0[u] - mx);
    sum += e[u];
  }
  sum = block_sum(sum, redv, 16);
  float best = -INFINITY;
  int besti = 0x7fffffff;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int v = tid + u * 1024;
    if (v < Ve) {
      const float pr = e[u] / sum;
      if (probs_row) probs_row[v] = pr;
      float q;
      if (q_row) {
        q = q_row[v];
      } else {
        const unsigned hsh =
            mix32s(mix32s((p.seed ^ nseed) + (unsigned)idx * 0x9E3779B9u) ^ (nlane << 16) ^ (unsigned)v);
        q = -logf(((float)(hsh >> 8) + 0.5f) * (1.0f / 16777216.0f));
      }
      const float s = pr / q;
      if (s > best || (s == best && v < besti)) { best = s; besti = v; }
    } else if (probs_row && v < V) {
      probs_row[v] = 0.f;
    }
  }
  const int tok = block_argmax(best, besti, redv, redi, 16);
  if constexpr (kLp) {
    const float ls = logf(sum);
    int own = tok;
    if constexpr (kForce) {
      if (ftok >= 0) own = ftok;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (tid + u * 1024 == own) *slp = x0[u] - mx - ls;
  }
  *amax_out = amax;
  return tok;
}

}  // namespace

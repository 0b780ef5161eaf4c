// s1 KV-cache decoding step (Text2SemanticDecoder.infer_panel_naive, t2s_model.py:762-863; T2SBlock.decode_next_token
// :186-222; sample / logits_to_probs, models/utils.py:118-160) for gfx950.
//
// One decoded token is a chain of batch-1 matrix-vector products over ~150 MB of weights plus attention over a growing
// key/value cache: HBM- and launch-bound, nothing for MFMA.  Laid out so that NOTHING about a step is a host argument:
//   * the key/value cache is preallocated [B][Lmax][E] and the current length lives in device memory (ctr[POS]) -- the
//     reference grows it with torch.cat every step;
//   * the step index, the number of generated tokens, the prompt length and the sampling seed are device state too
//     (ctr[IDX|YCOUNT|YLEN|SEED]);
//   * sampling (repetition penalty, nucleus cut, temperature, top-k, softmax, exponential-noise argmax), the EOS test,
//     the append to the token buffer and the embedding of the new token all run on the device.
// So the ~125 launches of a step are captured once into a HIP graph and replayed per token; the host only polls the stop
// flag every few steps.
//   dec_gemv   y = act(W . LN(a + r) + b): the post-LN residual of the previous sub-block is recomputed by every block in
//              its prologue (512 values) instead of being a launch of its own; block 0 stores it for the next residual.
//   dec_attn   one block per (batch, head): appends the new key/value to the cache, softmax(q.K/sqrt(d)).V over it.
//   dec_sample one block per batch row, 1024 threads, whole vocabulary (1025) in LDS, bitonic sort for the nucleus /
//              top-k pivots.
#include "s1_decode_common.h"

namespace {

constexpr int kMaxB = 4;

// ---- y[b][n] = act(bias[n] + sum_k W[n][k] * x[b][k]),  x = a  or  LayerNorm(a + r) --------------------------------
// A launch is a dependent chain of memory latencies, not a bandwidth problem (a workgroup touches 8-16 KB of weights), so
// the chain is kept as short as it gets: every weight load of the wave's rows is issued first (RPW x NPASS 16-byte loads
// in flight per lane), the input vector is staged -- and normalised with ONE block reduction of (sum, sum of squares) --
// while they are outstanding, then the dot products run out of registers and LDS.
template <typename T, int RPW, int NPASS>
__global__ __launch_bounds__(256) void dec_gemv(const T* __restrict__ W, const float* __restrict__ bias,
                                                const float* __restrict__ a, const float* __restrict__ r,
                                                const float* __restrict__ ln_g, const float* __restrict__ ln_b,
                                                float eps, float* x_out, float* __restrict__ y, int B, int N, int relu) {
  extern __shared__ float xs[];   // [B][K]
  __shared__ float red[8];
  constexpr int V = WVec<T>::V;
  constexpr int K = NPASS * 64 * V;
  constexpr int KPT = K / 256;     // input values per thread while staging
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = (blockIdx.x * 4 + wave) * RPW;
  uint4 w[RPW][NPASS];
#pragma unroll
  for (int i = 0; i < RPW; ++i)
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
      const int n = n0 + i;
      w[i][ps] = n < N ? *reinterpret_cast<const uint4*>(W + (long)n * K + (ps * 64 + lane) * V) : make_uint4(0, 0, 0, 0);
    }
  // everything the epilogues need is requested now as well: a load placed after a barrier starts a new latency
  float lg[KPT], lb[KPT], bz[RPW];
#pragma unroll
  for (int e = 0; e < KPT; ++e) {
    lg[e] = r ? ln_g[tid + e * 256] : 1.f;
    lb[e] = r ? ln_b[tid + e * 256] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < RPW; ++i) bz[i] = (bias && n0 + i < N) ? bias[n0 + i] : 0.f;
  for (int b = 0; b < B; ++b) {
    float v[KPT];
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int e = 0; e < KPT; ++e) {
      const int k = tid + e * 256;
      v[e] = a[b * K + k] + (r ? r[b * K + k] : 0.f);
      s += v[e];
      q += v[e] * v[e];
    }
    if (r) {
      s = wave_reduce_sum(s);
      q = wave_reduce_sum(q);
      __syncthreads();
      if (lane == 0) { red[wave] = s; red[4 + wave] = q; }
      __syncthreads();
      const float mu = (red[0] + red[1] + red[2] + red[3]) / K;
      const float var = fmaxf((red[4] + red[5] + red[6] + red[7]) / K - mu * mu, 0.f);
      const float rs = rsqrtf(var + eps);
#pragma unroll
      for (int e = 0; e < KPT; ++e) {
        const int k = tid + e * 256;
        v[e] = (v[e] - mu) * rs * lg[e] + lb[e];
        if (x_out && blockIdx.x == 0) x_out[b * K + k] = v[e];
      }
    }
#pragma unroll
    for (int e = 0; e < KPT; ++e) xs[b * K + tid + e * 256] = v[e];
  }
  __syncthreads();
  float acc[RPW][kMaxB];
#pragma unroll
  for (int i = 0; i < RPW; ++i)
#pragma unroll
    for (int b = 0; b < kMaxB; ++b) acc[i][b] = 0.f;
#pragma unroll
  for (int ps = 0; ps < NPASS; ++ps) {
    const int k0 = (ps * 64 + lane) * V;
#pragma unroll
    for (int b = 0; b < kMaxB; ++b) {
      if (b >= B) break;
      float xv[V];
#pragma unroll
      for (int e = 0; e < V; ++e) xv[e] = xs[b * K + k0 + e];
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        const T* pw = reinterpret_cast<const T*>(&w[i][ps]);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[i][b] += to_f<T>(pw[e]) * xv[e];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < RPW; ++i)
#pragma unroll
    for (int b = 0; b < kMaxB; ++b) {
      if (b >= B) break;
      const float sum = wave_reduce_sum(acc[i][b]);
      const int n = n0 + i;
      if (lane == 0 && n < N) {
        float o = sum + bz[i];
        if (relu) o = fmaxf(o, 0.f);
        y[(long)b * N + n] = o;
      }
    }
}

template <typename T, int D>
__global__ __launch_bounds__(256) void dec_attn(const float* __restrict__ qkv, T* kc, T* vc, const int* __restrict__ ctr,
                                                float* __restrict__ out, int H, int Lmax,
                                                const int* __restrict__ x_lens, int x_len) {
  extern __shared__ float sc[];   // [Lmax] scores -> probabilities
  __shared__ float qs[D], kn[D], vn[D], red[4], part[AttnShape<T, D>::G][D + 1];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / H, h = blockIdx.x % H, E = H * D;
  const int pos = ctr[EVT_DEC_POS];
  if (pos >= Lmax) return;            // cache full: the host bounds the number of steps, this only guards memory
  const int L = pos + 1;
  Prefetch<T, D> pf;
  pf.issue(kc, vc, b, h, E, Lmax, L, pos);
  if (tid < D) {
    const float* base = qkv + (long)b * 3 * E + h * D + tid;
    qs[tid] = base[0] * rsqrtf((float)D);
    const T kq = from_f<T>(base[E]), vq = from_f<T>(base[2 * E]);
    kn[tid] = to_f<T>(kq);
    vn[tid] = to_f<T>(vq);
    kc[((long)b * Lmax + pos) * E + h * D + tid] = kq;
    vc[((long)b * Lmax + pos) * E + h * D + tid] = vq;
  }
  __syncthreads();
  attn_tail<T, D>(pf, qs, kn, vn, sc, red, part, kc, vc, out, b, h, E, Lmax, L, pos, x_lens ? x_lens[b] : 0,
                  x_lens ? x_len : 0);
}

// ---- the same with the head's own rows of the packed in-projection computed in the launch -------------------------
// A workgroup (batch b, head h) needs only rows {q, k, v} x [h*D, (h+1)*D) of W_qkv: 3*D rows of E values (96 KB in
// bf16).  Computing them here removes the qkv launch of every block from the token step.  Input x = a or
// LayerNorm(a + r) as in dec_gemv (workgroups h == 0 store it to x_out).
template <typename T, int D, int NPASS>
__global__ __launch_bounds__(256) void dec_qkv_attn(const T* __restrict__ W, const float* __restrict__ bias,
                                                    const float* __restrict__ a, const float* __restrict__ r,
                                                    const float* __restrict__ ln_g, const float* __restrict__ ln_b,
                                                    float eps, float* x_out, T* kc, T* vc, const int* __restrict__ ctr,
                                                    float* __restrict__ out, int H, int Lmax,
                                                    const int* __restrict__ x_lens, int x_len) {
  extern __shared__ float sc[];   // [Lmax]
  constexpr int V = WVec<T>::V;
  constexpr int E = NPASS * 64 * V;       // model width == K of the projection
  constexpr int KPT = E / 256;
  constexpr int ROWS = 3 * D, RPWV = ROWS / 4;   // rows per wave
  constexpr int RC = NPASS == 1 ? RPWV : RPWV / 2;   // rows whose weights are in flight at once
  __shared__ float xs[E], proj[ROWS], qs[D], kn[D], vn[D], red[8], part[AttnShape<T, D>::G][D + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int pos = ctr[EVT_DEC_POS];
  if (pos >= Lmax) return;
  const int L = pos + 1;
  // projection row rho in [0, 3D): part = rho / D selects q / k / v, global row = part*E + h*D + rho % D
  auto grow = [&](int rho) { return (rho / D) * E + h * D + rho % D; };
  uint4 w[RC][NPASS];
#pragma unroll
  for (int i = 0; i < RC; ++i)
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps)
      w[i][ps] = *reinterpret_cast<const uint4*>(W + (long)grow(wave * RPWV + i) * E + (ps * 64 + lane) * V);
  Prefetch<T, D> pf;
  pf.issue(kc, vc, b, h, E, Lmax, L, pos);
  float lg[KPT], lb[KPT], v[KPT];
  float s = 0.f, q = 0.f;
#pragma unroll
  for (int e = 0; e < KPT; ++e) {
    const int k = tid + e * 256;
    lg[e] = r ? ln_g[k] : 1.f;
    lb[e] = r ? ln_b[k] : 0.f;
    v[e] = a[b * E + k] + (r ? r[b * E + k] : 0.f);
    s += v[e];
    q += v[e] * v[e];
  }
  const float bz = tid < ROWS ? bias[grow(tid)] : 0.f;
  if (r) {
    s = wave_reduce_sum(s);
    q = wave_reduce_sum(q);
    if (lane == 0) { red[wave] = s; red[4 + wave] = q; }
    __syncthreads();
    const float mu = (red[0] + red[1] + red[2] + red[3]) / E;
    const float var = fmaxf((red[4] + red[5] + red[6] + red[7]) / E - mu * mu, 0.f);
    const float rs = rsqrtf(var + eps);
#pragma unroll
    for (int e = 0; e < KPT; ++e) {
      v[e] = (v[e] - mu) * rs * lg[e] + lb[e];
      if (x_out && h == 0) x_out[b * E + tid + e * 256] = v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < KPT; ++e) xs[tid + e * 256] = v[e];
  __syncthreads();
#pragma unroll
  for (int chunk = 0; chunk < RPWV / RC; ++chunk) {
    if (chunk > 0) {
#pragma unroll
      for (int i = 0; i < RC; ++i)
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps)
          w[i][ps] = *reinterpret_cast<const uint4*>(W + (long)grow(wave * RPWV + chunk * RC + i) * E + (ps * 64 + lane) * V);
    }
#pragma unroll
    for (int i = 0; i < RC; ++i) {
      float acc = 0.f;
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps) {
        const T* pw = reinterpret_cast<const T*>(&w[i][ps]);
        const int k0 = (ps * 64 + lane) * V;
#pragma unroll
        for (int e = 0; e < V; ++e) acc += to_f<T>(pw[e]) * xs[k0 + e];
      }
      acc = wave_reduce_sum(acc);
      if (lane == 0) proj[wave * RPWV + chunk * RC + i] = acc;
    }
  }
  __syncthreads();
  if (tid < ROWS) proj[tid] += bz;
  __syncthreads();
  if (tid < D) {
    qs[tid] = proj[tid] * rsqrtf((float)D);
    const T kq = from_f<T>(proj[D + tid]), vq = from_f<T>(proj[2 * D + tid]);
    kn[tid] = to_f<T>(kq);
    vn[tid] = to_f<T>(vq);
    kc[((long)b * Lmax + pos) * E + h * D + tid] = kq;
    vc[((long)b * Lmax + pos) * E + h * D + tid] = vq;
  }
  __syncthreads();
  attn_tail<T, D>(pf, qs, kn, vn, sc, red, part, kc, vc, out, b, h, E, Lmax, L, pos, x_lens ? x_lens[b] : 0,
                  x_lens ? x_len : 0);
}

// ---- sampling ---------------------------------------------------------------------------------------------------
struct EmbedArgs {          // optional tail of dec_sample: x_next and the counter update of the step (B == 1 only)
  const float* emb; const float* pe; const float* alpha; float* x; float x_scale; int E, npos, dpos;
};

__global__ __launch_bounds__(1024) void dec_sample(evt_sample_params p, const float* __restrict__ logits, long* y,
                                                   int* ctr, const float* __restrict__ noise, int* stop_idx,
                                                   float* probs_out, EmbedArgs ea, const int* __restrict__ row_seed) {
  const int tid = threadIdx.x, b = blockIdx.x, V = p.V;
  const int idx = ctr[EVT_DEC_IDX], ycount = ctr[EVT_DEC_YCOUNT];
  // built-in noise of this row: (seed, lane) from the row-seed table, else (ctr[SEED], b)
  const unsigned nseed = row_seed ? (unsigned)row_seed[2 * b] : (unsigned)ctr[EVT_DEC_SEED];
  const unsigned nlane = row_seed ? (unsigned)row_seed[2 * b + 1] : (unsigned)b;
  long* yb = y + (long)b * p.ymax;
  int amax;
  const int tok = sample_row(p, logits + (long)b * V, yb, idx, ycount, nseed, nlane,
                             noise ? noise + ((long)idx * p.noise_rows + (p.noise_rows > 1 ? b : 0)) * V : nullptr,
                             probs_out ? probs_out + (long)b * V : nullptr, &amax);
  if (tid == 0) {
    if (ycount < p.ymax) yb[ycount] = tok;
    if ((amax == p.eos || tok == p.eos) && stop_idx[b] < 0) stop_idx[b] = idx;
  }
  if (ea.x) {       // x_next = emb[token] * x_scale + alpha * pe[y_len + idx], then the step's counter update
    int ppos = ctr[EVT_DEC_YLEN] + idx;
    if (ppos >= ea.npos) ppos = ea.npos - 1;
    const float al = ea.alpha[0];
    for (int c = tid; c < ea.E; c += 1024)
      ea.x[(long)b * ea.E + c] = ea.emb[(long)tok * ea.E + c] * ea.x_scale + al * ea.pe[(long)ppos * ea.E + c];
    __syncthreads();     // every read of ctr[] above is done (single workgroup: the launcher checks B == 1)
    if (tid == 0) {
      ctr[EVT_DEC_POS] += ea.dpos;
      ctr[EVT_DEC_IDX] = idx + 1;
      ctr[EVT_DEC_YCOUNT] = ycount + 1;
    }
  }
}

// ---- x_next = emb[token] * x_scale + alpha * pe[y_len + idx]  (t2s_model.py:860-861) ----------------------------
__global__ __launch_bounds__(256) void dec_embed(const float* __restrict__ emb, const float* __restrict__ pe,
                                                 const float* __restrict__ alpha, float x_scale,
                                                 const long* __restrict__ y, const int* __restrict__ ctr,
                                                 float* __restrict__ x, int E, int ymax, int npos) {
  const int b = blockIdx.x;
  const int idx = ctr[EVT_DEC_IDX], ycount = ctr[EVT_DEC_YCOUNT], ylen = ctr[EVT_DEC_YLEN];
  const long tok = y[(long)b * ymax + (ycount < ymax ? ycount : ymax - 1)];
  int ppos = ylen + idx;
  if (ppos >= npos) ppos = npos - 1;
  const float al = alpha[0];
  for (int c = threadIdx.x; c < E; c += 256) x[(long)b * E + c] = emb[tok * E + c] * x_scale + al * pe[(long)ppos * E + c];
}

__global__ void dec_advance(int* ctr, int dpos) {
  ctr[EVT_DEC_POS] += dpos;
  ctr[EVT_DEC_IDX] += 1;
  ctr[EVT_DEC_YCOUNT] += 1;
}

}  // namespace

template <typename T>
static int launch_gemv(const void* W, const float* bias, const float* a, const float* r, const float* g, const float* bt,
                       float eps, float* x_out, float* y, int B, int N, int K, int relu, hipStream_t st) {
  constexpr int V = WVec<T>::V;
  const size_t shm = (size_t)B * K * sizeof(float);
  const int npass = K / (64 * V);
  // rows per wave: keep >= ~128 workgroups in flight for the short matrices, two rows per wave for the tall ones
  const int rpw = N >= 1024 ? 2 : 1;
  const int blocks = (N + 4 * rpw - 1) / (4 * rpw);
#define EVT_GEMV(RPW, NP)                                                                                            \
  hipLaunchKernelGGL((dec_gemv<T, RPW, NP>), dim3(blocks), dim3(256), shm, st, (const T*)W, bias, a, r, g, bt, eps, \
                     x_out, y, B, N, relu)
  if (npass * 64 * V != K) return EVT_ENOTSUP;
  if (rpw == 2) {
    if (npass == 1) EVT_GEMV(2, 1); else if (npass == 2) EVT_GEMV(2, 2); else if (npass == 4) EVT_GEMV(2, 4);
    else if (npass == 8) EVT_GEMV(2, 8); else return EVT_ENOTSUP;
  } else {
    if (npass == 1) EVT_GEMV(1, 1); else if (npass == 2) EVT_GEMV(1, 2); else if (npass == 4) EVT_GEMV(1, 4);
    else if (npass == 8) EVT_GEMV(1, 8); else return EVT_ENOTSUP;
  }
#undef EVT_GEMV
  return evt_check_launch();
}

// The host side of evt_dec_sample, evt_dec_sample_rows and evt_dec_sample_embed around the one kernel dec_sample.  With
// an embedding tail (ea.x set: evt_dec_sample_embed) the kernel moves the counters itself, which only a single workgroup
// may do: the caller passes B = 1, and the one row reads column 0 of an injected noise table.
static int launch_sample(const evt_sample_params* p, const float* logits, int64_t* y, const int32_t* ctr,
                         const float* noise, int32_t* stop_idx, float* probs_out, EmbedArgs ea, const int32_t* row_seed,
                         int32_t B, void* stream) {
  if (!p || !logits || !y || !ctr || !stop_idx || B <= 0) return EVT_EINVAL;
  if (p->V <= 1 || p->V > kSortN || p->ymax <= 0 || p->repetition_penalty <= 0.f) return EVT_EINVAL;
  evt_sample_params sp = *p;
  if (sp.noise_rows < 1 || ea.x) sp.noise_rows = 1;
  hipLaunchKernelGGL(dec_sample, dim3(B), dim3(1024), 0, (hipStream_t)stream, sp, logits, (long*)y, (int*)ctr, noise,
                     stop_idx, probs_out, ea, row_seed);
  return evt_check_launch();
}

extern "C" {

int evt_dec_gemv(int32_t wdtype, const void* W, const float* bias, const float* a, const float* r, const float* ln_g,
                 const float* ln_b, float ln_eps, float* x_out, float* y, int32_t B, int32_t N, int32_t K, int32_t relu,
                 void* stream) {
  if (!W || !a || !y || B <= 0 || N <= 0 || K <= 0) return EVT_EINVAL;
  if (r && (!ln_g || !ln_b)) return EVT_EINVAL;
  if (B > kMaxB || K % 512 || (size_t)B * K * 4 > 64 * 1024) return EVT_ENOTSUP;
  hipStream_t st = (hipStream_t)stream;
  if (wdtype == EVT_DT_HALF) return launch_gemv<h16_t>(W, bias, a, r, ln_g, ln_b, ln_eps, x_out, y, B, N, K, relu, st);
  if (wdtype == EVT_DT_F32) return launch_gemv<float>(W, bias, a, r, ln_g, ln_b, ln_eps, x_out, y, B, N, K, relu, st);
  return EVT_EINVAL;
}

int evt_dec_attn(int32_t cdtype, const float* qkv, void* kcache, void* vcache, const int32_t* ctr, float* out, int32_t B,
                 int32_t H, int32_t D, int32_t Lmax, const int32_t* x_lens, int32_t x_len, void* stream) {
  if (!qkv || !kcache || !vcache || !ctr || !out || B <= 0 || H <= 0 || Lmax <= 0) return EVT_EINVAL;
  if (D != 32 || (size_t)Lmax * 4 > 60 * 1024) return EVT_ENOTSUP;
  const size_t shm = (size_t)Lmax * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (cdtype == EVT_DT_HALF)
    hipLaunchKernelGGL((dec_attn<h16_t, 32>), dim3(B * H), dim3(256), shm, st, qkv, (h16_t*)kcache, (h16_t*)vcache,
                       (const int*)ctr, out, H, Lmax, (const int*)x_lens, x_len);
  else if (cdtype == EVT_DT_F32)
    hipLaunchKernelGGL((dec_attn<float, 32>), dim3(B * H), dim3(256), shm, st, qkv, (float*)kcache, (float*)vcache,
                       (const int*)ctr, out, H, Lmax, (const int*)x_lens, x_len);
  else return EVT_EINVAL;
  return evt_check_launch();
}

int evt_dec_sample(const evt_sample_params* p, const float* logits, int64_t* y, const int32_t* ctr, const float* noise,
                   int32_t* stop_idx, float* probs_out, int32_t B, void* stream) {
  return launch_sample(p, logits, y, ctr, noise, stop_idx, probs_out, EmbedArgs{}, nullptr, B, stream);
}

int evt_dec_sample_rows(const evt_sample_params* p, const float* logits, int64_t* y, const int32_t* ctr,
                        const float* noise, int32_t* stop_idx, float* probs_out, const int32_t* row_seed, int32_t B,
                        void* stream) {
  if (!row_seed) return EVT_EINVAL;
  return launch_sample(p, logits, y, ctr, noise, stop_idx, probs_out, EmbedArgs{}, row_seed, B, stream);
}

int evt_dec_sample_embed(const evt_sample_params* p, const float* logits, int64_t* y, int32_t* ctr, const float* noise,
                         int32_t* stop_idx, const float* emb, const float* pe, const float* alpha, float x_scale, float* x,
                         int32_t E, int32_t npos, int32_t dpos, void* stream) {
  if (!emb || !pe || !alpha || !x || E <= 0 || npos <= 0) return EVT_EINVAL;
  return launch_sample(p, logits, y, ctr, noise, stop_idx, nullptr, EmbedArgs{emb, pe, alpha, x, x_scale, E, npos, dpos},
                       nullptr, 1, stream);
}

int evt_dec_qkv_attn(int32_t dtype, const void* Wqkv, const float* bqkv, const float* a, const float* r,
                     const float* ln_g, const float* ln_b, float ln_eps, float* x_out, void* kcache, void* vcache,
                     const int32_t* ctr, float* out, int32_t B, int32_t H, int32_t D, int32_t Lmax, const int32_t* x_lens,
                     int32_t x_len, void* stream) {
  if (!Wqkv || !bqkv || !a || !kcache || !vcache || !ctr || !out || B <= 0 || H <= 0 || Lmax <= 0) return EVT_EINVAL;
  if (r && (!ln_g || !ln_b)) return EVT_EINVAL;
  if (D != 32 || H * D != 512 || (size_t)Lmax * 4 > 48 * 1024) return EVT_ENOTSUP;
  const size_t shm = (size_t)Lmax * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EVT_DT_HALF)
    hipLaunchKernelGGL((dec_qkv_attn<h16_t, 32, 1>), dim3(B * H), dim3(256), shm, st, (const h16_t*)Wqkv, bqkv, a, r,
                       ln_g, ln_b, ln_eps, x_out, (h16_t*)kcache, (h16_t*)vcache, (const int*)ctr, out, H, Lmax,
                       (const int*)x_lens, x_len);
  else if (dtype == EVT_DT_F32)
    hipLaunchKernelGGL((dec_qkv_attn<float, 32, 2>), dim3(B * H), dim3(256), shm, st, (const float*)Wqkv, bqkv, a, r,
                       ln_g, ln_b, ln_eps, x_out, (float*)kcache, (float*)vcache, (const int*)ctr, out, H, Lmax,
                       (const int*)x_lens, x_len);
  else return EVT_EINVAL;
  return evt_check_launch();
}

int evt_dec_embed(const float* emb, const float* pe, const float* alpha, float x_scale, const int64_t* y,
                  const int32_t* ctr, float* x, int32_t B, int32_t E, int32_t ymax, int32_t npos, void* stream) {
  if (!emb || !pe || !alpha || !y || !ctr || !x || B <= 0 || E <= 0 || ymax <= 0 || npos <= 0) return EVT_EINVAL;
  hipLaunchKernelGGL(dec_embed, dim3(B), dim3(256), 0, (hipStream_t)stream, emb, pe, alpha, x_scale, (const long*)y,
                     (const int*)ctr, x, E, ymax, npos);
  return evt_check_launch();
}

int evt_dec_advance(int32_t* ctr, int32_t dpos, void* stream) {
  if (!ctr) return EVT_EINVAL;
  hipLaunchKernelGGL(dec_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, (int*)ctr, dpos);
  return evt_check_launch();
}

}  // extern "C"

// Degenerate Conv1d shapes of the s2 path that have no GEMM in them (gfx950):
//   * Cout == 1  (HiFi-GAN conv_post 16->1 k7, models.py:446; discriminator conv_post 1024->1 k3, models.py:536,574):
//     a dot product per output position  -> lane groups reduce over (tap, channel) with 16-byte loads;
//     its weight gradient is a dy-weighted sum of input rows -> per-thread register accumulators.
//   * Cin == 1   (discriminator first layers 1->16 k15 / 1->32 k5 s3, models.py:490-497,566): forward = a k-tap FIR per
//     output channel from an LDS-staged signal segment (8 channels = one 16-byte store per thread); in both backward
//     kernels a thread owns 8 channels with up to 16 taps in registers and streams dy_eff through registers in 16-byte
//     pieces: backward-data leaves the k tap sums of every dy row in LDS and adds the ones that hit each input sample; the
//     weight gradient accumulates KM x 8 tap sums per thread against the LDS-staged signal.
// HBM-bound byte work: coalesced 16-byte reads, LDS only for the small weight vector / block reduction.  Weight gradients
// leave one scratch row [image | bias sums] per block and ONE fold launch (fold.hip) adds the rows in a fixed order.
#include "evt_common.h"
#include "../../include/evt.h"
#include "conv_p.h"

namespace {

struct SP {
  const void* x; const void* w; const float* bias; const void* y_in; const void* dy; void* y; float* dw;
  int nseq, lin, lout, cin, cout, k, stride, pad, dil;
  int ck, nchunk, kp;   // REG geometry
  float in_slope; int out_act; float out_slope;
  int G;                // lanes per output (power of two <= 64)
  int pos_per_block;
  float* ws;            // scratch rows for the per-block partial results (fold.hip), or null: fp32 atomics
  long ws_row;          // floats per scratch row
  float* dbias;         // Cout == 1 weight gradient: the bias gradient is summed by the same kernel (or null)
  int tile;             // cin1_bwd_data: inputs per tile
  int step_q, step_r;   // cin1_bwd_weight: the grid's stride in tiles as quotient and remainder by the tiles per sequence
};

__device__ __forceinline__ long sreg_index(const SP& p, int d0, int d1, int t) {
  const int chunk = d1 / p.ck, cc = d1 - chunk * p.ck;
  return (((long)d0 * p.nchunk + chunk) * p.kp + t) * p.ck + cc;
}

// position r of a flattened [n][len] index space as (n, i): one division where a walk starts, additions afterwards
struct Walk { int seq, i; };
__device__ __forceinline__ Walk walk_at(long r, int len) {
  Walk w;
  w.seq = (int)(r / len);
  w.i = (int)(r - (long)w.seq * len);
  return w;
}
__device__ __forceinline__ void walk_add(Walk& w, int dq, int dr, int len) {
  w.seq += dq; w.i += dr;
  if (w.i >= len) { w.i -= len; ++w.seq; }
}

// 8 consecutive channels of a [Cout]-wide row: one 16-byte load for the 16-bit types, two for fp32
template <typename T> struct Raw8 { uint4 q[sizeof(T) / 2]; };
template <typename T> __device__ __forceinline__ Raw8<T> ld8(const T* s) {
  Raw8<T> r;
#pragma unroll
  for (int i = 0; i < (int)sizeof(T) / 2; ++i) r.q[i] = reinterpret_cast<const uint4*>(s)[i];
  return r;
}
template <typename T> __device__ __forceinline__ void cvt8(const Raw8<T>& r, float* f) {
  const T* pv = reinterpret_cast<const T*>(&r);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = to_f<T>(pv[e]);
}

// ---- Cout == 1 forward: G lanes per output --------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void cout1_fwd(SP p) {
  constexpr int V = 16 / sizeof(T);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* wl = reinterpret_cast<float*>(smem);   // [k][cin] fp32
  const T* w = reinterpret_cast<const T*>(p.w);
  for (int i = threadIdx.x; i < p.k * p.cin; i += 256) {
    const int t = i / p.cin, c = i - t * p.cin;
    wl[i] = to_f<T>(w[sreg_index(p, 0, c, t)]);
  }
  __syncthreads();
  const int G = p.G;
  const int sub = threadIdx.x % G;
  const long gid = ((long)blockIdx.x * 256 + threadIdx.x) / G;
  const long ngroups = (long)gridDim.x * 256 / G;
  const long total = (long)p.nseq * p.lout;
  const int ppr = p.cin / V;             // 16-byte pieces per row
  const int pieces = p.k * ppr;
  const T* x = reinterpret_cast<const T*>(p.x);
  const long rounds = (total + ngroups - 1) / ngroups;
  for (long rd = 0; rd < rounds; ++rd) {   // uniform trip count: the shuffles below need every lane
    const long o = rd * ngroups + gid;
    const bool live = o < total;
    const int q = live ? (int)(o % p.lout) : 0;
    const int seq = live ? (int)(o / p.lout) : 0;
    float acc = 0.f;
    if (live) {
      for (int pc = sub; pc < pieces; pc += G) {
        const int t = pc / ppr, c0 = (pc - t * ppr) * V;
        const int row = q * p.stride + t * p.dil - p.pad;
        if (row < 0 || row >= p.lin) continue;
        const uint4 v = *reinterpret_cast<const uint4*>(x + ((long)seq * p.lin + row) * p.cin + c0);
        const T* pv = reinterpret_cast<const T*>(&v);
        const float* wr = wl + t * p.cin + c0;
#pragma unroll
        for (int e = 0; e < V; ++e) acc += lrelu_f(to_f<T>(pv[e]), p.in_slope) * wr[e];
      }
    }
    for (int off = G >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (live && sub == 0) {
      if (p.bias) acc += p.bias[0];
      if (p.out_act == EVT_ACT_LRELU) acc = lrelu_f(acc, p.out_slope);
      else if (p.out_act == EVT_ACT_TANH) acc = tanhf(acc);
      reinterpret_cast<T*>(p.y)[o] = from_f<T>(acc);
    }
  }
}

// ---- Cout == 1 weight gradients: what the two kernels share ---------------------------------------------------------------
// sum of dy_eff over the outputs [o0, o1): the block's share of the bias gradient (the kernels load dy_eff anyway; this is
// 2 bytes per output next to the rows of [Cin] they stream)
template <typename T>
__device__ __forceinline__ float cout1_dy_sum(const SP& p, long o0, long o1) {
  __shared__ float redb[4];
  const T* dy = reinterpret_cast<const T*>(p.dy);
  const T* ys = reinterpret_cast<const T*>(p.y_in);
  float s = 0.f;
  for (long o = o0 + threadIdx.x; o < o1; o += 256) {
    float d = to_f<T>(dy[o]);
    if (ys) d *= dact_from_out(p.out_act, to_f<T>(ys[o]), p.out_slope);
    s += d;
  }
  return block_reduce_sum_256(s, redb);
}

// red = [npl][k * cin] partial sums of the block's row lanes: added in lane order (LDS atomics would add them in arrival
// order: last bits that change from run to run) and stored as one scratch row [whole REG image | bias sum] -- the image's
// padded entries as zeros, so that one fold launch can add whole rows --, or added to dw / dbias with atomics without scratch
__device__ __forceinline__ void cout1_store_partial(const SP& p, const float* red, int npl, float bsum) {
  const int kc = p.k * p.cin;
  const int img = p.nchunk * p.kp * p.ck;
  for (int i = threadIdx.x; i < img; i += 256) {
    const int run = i / p.ck, cc = i - run * p.ck;
    const int chunk = run / p.kp, t = run - chunk * p.kp;
    const int c = chunk * p.ck + cc;
    const bool real = t < p.k && c < p.cin;
    float v = 0.f;
    if (real) {
      v = red[t * p.cin + c];
      for (int l = 1; l < npl; ++l) v += red[l * kc + t * p.cin + c];
    }
    if (p.ws) p.ws[(long)blockIdx.x * p.ws_row + i] = v;
    else if (real) atomicAdd(p.dw + i, v);
  }
  if (threadIdx.x == 0 && p.dbias) {
    if (p.ws) p.ws[(long)blockIdx.x * p.ws_row + img] = bsum;
    else atomicAdd(p.dbias, bsum);
  }
}

// ---- Cout == 1 backward-weight: dW[t][c] += sum_pos dy_eff[pos] * lrelu(x)[row(pos,t)][c] --------------------
// thread -> (position lane pl, piece pc); up to NA pieces per thread; block covers pos_per_block positions
template <typename T>
__global__ __launch_bounds__(256) void cout1_bwd_weight(SP p) {
  constexpr int V = 16 / sizeof(T);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* red = reinterpret_cast<float*>(smem);   // [npl][k*cin]
  const int ppr = p.cin / V;
  const int pieces = p.k * ppr;
  int pp = 1;
  while (pp < pieces && pp < 256) pp <<= 1;       // pieces padded to a power of two (<= 256)
  const int npl = 256 / pp;                        // positions processed in parallel
  const int pl = threadIdx.x / pp, pc0 = threadIdx.x % pp;
  constexpr int NA = 4;   // k*cin <= 4096 (evt_small_kind) -> at most 1024 pieces -> 4 per thread
  float acc[NA][V];
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int e = 0; e < V; ++e) acc[a][e] = 0.f;
  const T* x = reinterpret_cast<const T*>(p.x);
  const T* dy = reinterpret_cast<const T*>(p.dy);
  const T* ys = reinterpret_cast<const T*>(p.y_in);
  const long total = (long)p.nseq * p.lout;
  const long p0 = (long)blockIdx.x * p.pos_per_block;
  const long p1 = min(total, p0 + p.pos_per_block);
  // UP positions per trip: all their 16-byte loads are issued before the first use (the loop is latency-bound)
  constexpr int UP = 4;
  for (long ob = p0 + pl; ob < p1; ob += (long)npl * UP) {
    uint4 v[UP][NA];
    float d[UP];
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      const long o = ob + (long)u * npl;
      const bool live = o < p1;
      const int q = live ? (int)(o % p.lout) : 0, seq = live ? (int)(o / p.lout) : 0;
      d[u] = live ? to_f<T>(dy[o]) : 0.f;
      if (live && ys) d[u] *= dact_from_out(p.out_act, to_f<T>(ys[o]), p.out_slope);
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int pc = pc0 + a * pp;
        const int t = pc / ppr, c0 = (pc - t * ppr) * V;
        const int row = q * p.stride + t * p.dil - p.pad;
        const bool ok = live && pc < pieces && row >= 0 && row < p.lin;
        v[u][a] = ok ? *reinterpret_cast<const uint4*>(x + ((long)seq * p.lin + row) * p.cin + c0) : make_uint4(0, 0, 0, 0);
      }
    }
#pragma unroll
    for (int u = 0; u < UP; ++u)
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const T* pv = reinterpret_cast<const T*>(&v[u][a]);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[a][e] += d[u] * lrelu_f(to_f<T>(pv[e]), p.in_slope);
      }
  }
  const int kc = p.k * p.cin;
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int pc = pc0 + a * pp;
    if (pc < pieces) {
      const int t = pc / ppr, c0 = (pc - t * ppr) * V;
#pragma unroll
      for (int e = 0; e < V; ++e) red[pl * kc + t * p.cin + c0 + e] = acc[a][e];
    }
  }
  const float bsum = p.dbias ? cout1_dy_sum<T>(p, p0, p1) : 0.f;
  __syncthreads();
  cout1_store_partial(p, red, npl, bsum);
}

// ---- Cin == 1 forward: y[q][co] = act(b[co] + sum_t w[co][t] * lrelu(x)[q*s + t*dil - pad]) ---------------------
// block = TP consecutive outputs of one sequence; thread = 8 channels of one position per pass
constexpr int C1_TP = 512;

template <typename T>
__global__ __launch_bounds__(256) void cin1_fwd(SP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* wl = reinterpret_cast<float*>(smem);            // [k][cout]
  float* xl = wl + p.k * p.cout;                          // signal segment
  const T* w = reinterpret_cast<const T*>(p.w);
  for (int i = threadIdx.x; i < p.k * p.cout; i += 256) {
    const int t = i / p.cout, co = i - t * p.cout;
    wl[i] = to_f<T>(w[sreg_index(p, co, 0, t)]);
  }
  const int tiles = (p.lout + C1_TP - 1) / C1_TP;
  const int seq = blockIdx.x / tiles, q0 = (blockIdx.x - seq * tiles) * C1_TP;
  const int nq = min(C1_TP, p.lout - q0);
  const int seg = (nq - 1) * p.stride + (p.k - 1) * p.dil + 1;
  const int r0 = q0 * p.stride - p.pad;
  const T* x = reinterpret_cast<const T*>(p.x) + (long)seq * p.lin;
  for (int i = threadIdx.x; i < seg; i += 256) {
    const int r = r0 + i;
    xl[i] = (r >= 0 && r < p.lin) ? lrelu_f(to_f<T>(x[r]), p.in_slope) : 0.f;
  }
  __syncthreads();
  const int CG = p.cout >> 3, ppp = 256 / CG;
  const int c0 = (threadIdx.x % CG) * 8;
  float bv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bv[e] = p.bias ? p.bias[c0 + e] : 0.f;
  T* y = reinterpret_cast<T*>(p.y) + ((long)seq * p.lout + q0) * p.cout;
  for (int q = threadIdx.x / CG; q < nq; q += ppp) {
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = bv[e];
    for (int t = 0; t < p.k; ++t) {
      const float xv = xl[q * p.stride + t * p.dil];
      const float4 w0 = *reinterpret_cast<const float4*>(wl + t * p.cout + c0);
      const float4 w1 = *reinterpret_cast<const float4*>(wl + t * p.cout + c0 + 4);
      acc[0] += xv * w0.x; acc[1] += xv * w0.y; acc[2] += xv * w0.z; acc[3] += xv * w0.w;
      acc[4] += xv * w1.x; acc[5] += xv * w1.y; acc[6] += xv * w1.z; acc[7] += xv * w1.w;
    }
    T outv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = acc[e];
      if (p.out_act == EVT_ACT_LRELU) v = lrelu_f(v, p.out_slope);
      else if (p.out_act == EVT_ACT_TANH) v = tanhf(v);
      outv[e] = from_f<T>(v);
    }
    T* dst = y + (long)q * p.cout + c0;
    if constexpr (sizeof(T) == 2) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<uint4*>(outv);
    else { reinterpret_cast<float4*>(dst)[0] = reinterpret_cast<float4*>(outv)[0]; reinterpret_cast<float4*>(dst)[1] = reinterpret_cast<float4*>(outv)[1]; }
  }
}

// wl[t][co] fp32 from the image [co][kp] (cin = 1: ck = nchunk = 1), read in image order
template <typename T>
__device__ __forceinline__ void cin1_fill_wl(const SP& p, float* wl) {
  const T* w = reinterpret_cast<const T*>(p.w);
  for (int i = threadIdx.x; i < p.cout * p.kp; i += 256) {
    const int co = i / p.kp, t = i - co * p.kp;
    if (t < p.k) wl[t * p.cout + co] = to_f<T>(w[i]);
  }
}

// taps t0 .. t0 + KM of the thread's 8 channels, from the LDS table
template <int KM>
__device__ __forceinline__ void cin1_taps(const SP& p, const float* wl, int c0, int t0, float (&wf)[KM][8]) {
#pragma unroll
  for (int t = 0; t < KM; ++t) {
    const bool ok = t0 + t < p.k;
    const float4 w0 = ok ? *reinterpret_cast<const float4*>(wl + (t0 + t) * p.cout + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 w1 = ok ? *reinterpret_cast<const float4*>(wl + (t0 + t) * p.cout + c0 + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    wf[t][0] = w0.x; wf[t][1] = w0.y; wf[t][2] = w0.z; wf[t][3] = w0.w;
    wf[t][4] = w1.x; wf[t][5] = w1.y; wf[t][6] = w1.z; wf[t][7] = w1.w;
  }
}

constexpr int C1_TI = 512;   // inputs per backward-data tile (halved by the launcher while the tile's LDS image is too big)

// ---- Cin == 1 backward-data: dx[i] = sum_t sum_co dy_eff[(i + pad - t*dil)/s][co] * w[co][t] (exact multiples only) --
// block = p.tile consecutive inputs of one sequence and the dy rows that reach them.  Phase 1 is dy-stationary: a thread
// takes 8 channels of a row from global memory and leaves their k tap dot products in LDS (pl[row][channel group][t]);
// phase 2 adds, per input sample, the (row, t) pairs that hit it over the channel groups.
template <typename T, int KM>
__global__ __launch_bounds__(256) void cin1_bwd_data(SP p, const void* gate, const void* dx_add) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* wl = reinterpret_cast<float*>(smem);            // [k][cout]
  float* pl = wl + p.k * p.cout;                          // [rows][CG][k]
  cin1_fill_wl<T>(p, wl);
  const int TI = p.tile;
  const int tiles = (p.lin + TI - 1) / TI;
  const int seq = blockIdx.x / tiles, i0 = (blockIdx.x - seq * tiles) * TI;
  const int ni = min(TI, p.lin - i0);
  // output rows q that can touch inputs [i0, i0 + ni): q*s - pad + t*dil = i
  int qlo = i0 + p.pad - (p.k - 1) * p.dil;
  qlo = qlo <= 0 ? 0 : (qlo + p.stride - 1) / p.stride;
  int qhi = (i0 + ni - 1 + p.pad) / p.stride;
  if (qhi > p.lout - 1) qhi = p.lout - 1;
  const int nrows = qhi - qlo + 1;
  const int CG = p.cout >> 3, ppp = 256 / CG;
  const int cg = threadIdx.x & (CG - 1), c0 = cg * 8, rl = threadIdx.x / CG;
  const T* dy = reinterpret_cast<const T*>(p.dy) + ((long)seq * p.lout + qlo) * p.cout + c0;
  const T* ys = p.y_in ? reinterpret_cast<const T*>(p.y_in) + ((long)seq * p.lout + qlo) * p.cout + c0 : nullptr;
  __syncthreads();
  constexpr int UP = 4;
  for (int t0 = 0; t0 < p.k; t0 += KM) {                  // one pass unless k > KM
    float wf[KM][8];
    cin1_taps<KM>(p, wl, c0, t0, wf);
    for (int rb = rl; rb < nrows; rb += ppp * UP) {
      Raw8<T> v[UP], va[UP];
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        const int r = rb + u * ppp;
        if (r < nrows) {
          v[u] = ld8<T>(dy + (long)r * p.cout);
          if (ys) va[u] = ld8<T>(ys + (long)r * p.cout);
        }
      }
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        const int r = rb + u * ppp;
        if (r < nrows) {
          float d[8], a[8];
          cvt8<T>(v[u], d);
          if (ys) {
            cvt8<T>(va[u], a);
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] *= dact_from_out(p.out_act, a[e], p.out_slope);
          }
          float* dst = pl + ((long)r * CG + cg) * p.k + t0;
#pragma unroll
          for (int t = 0; t < KM; ++t) {
            if (t0 + t < p.k) {
              float s = 0.f;
#pragma unroll
              for (int e = 0; e < 8; ++e) s += d[e] * wf[t][e];
              dst[t] = s;
            }
          }
        }
      }
    }
  }
  __syncthreads();
  T* dx = reinterpret_cast<T*>(p.y) + (long)seq * p.lin;
  const T* gt = gate ? reinterpret_cast<const T*>(gate) + (long)seq * p.lin : nullptr;
  const T* ad = dx_add ? reinterpret_cast<const T*>(dx_add) + (long)seq * p.lin : nullptr;
  for (int ii = threadIdx.x; ii < ni; ii += 256) {
    const int i = i0 + ii;
    float acc = 0.f;
    for (int t = 0; t < p.k; ++t) {
      const int j = i + p.pad - t * p.dil;
      if (j < 0) break;
      const int q = j / p.stride;
      if (q * p.stride != j || q > qhi || q < qlo) continue;
      const float* pr = pl + (long)(q - qlo) * CG * p.k + t;
      float s = pr[0];
      for (int g = 1; g < CG; ++g) s += pr[g * p.k];
      acc += s;
    }
    if (gt) acc *= (to_f<T>(gt[i]) > 0.f ? 1.f : p.in_slope);
    if (ad) acc += to_f<T>(ad[i]);
    dx[i] = from_f<T>(acc);
  }
}

constexpr int C1_TQ = 256;   // outputs per weight-gradient tile

// ---- Cin == 1 backward-weight: dW[co][t] += sum_pos dy_eff[pos][co] * lrelu(x)[pos*s + t*dil - pad]; dbias fused ----
// Blocks stride over tiles of C1_TQ outputs of one sequence.  Per tile the signal segment is staged in LDS; a thread
// streams 8 channels of dy_eff of every (256 / CG)-th position through registers into KM x 8 tap accumulators (+ 8 bias
// sums).  At the end the lanes that share a channel group meet by shuffles, the four waves in LDS, in a fixed order.
template <typename T, int KM>
__global__ __launch_bounds__(256) void cin1_bwd_weight(SP p, float* dbias) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* xl = reinterpret_cast<float*>(smem);            // signal segment
  __shared__ float red[4][4][(KM + 1) * 8];               // [wave][channel group][tap (KM: bias)][8]
  const int CG = p.cout >> 3, ppp = 256 / CG;
  const int cg = threadIdx.x & (CG - 1), c0 = cg * 8, ql = threadIdx.x / CG;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles = (p.lout + C1_TQ - 1) / C1_TQ;
  const long ntiles = (long)p.nseq * tiles;
  constexpr int UP = KM <= 8 ? 4 : 2;
  for (int t0 = 0; t0 < p.k; t0 += KM) {                  // one pass unless k > KM
    float acc[KM][8], bacc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      bacc[e] = 0.f;
#pragma unroll
      for (int t = 0; t < KM; ++t) acc[t][e] = 0.f;
    }
    Walk wk = walk_at(blockIdx.x, tiles);                 // (sequence, tile of the sequence)
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const int q0 = wk.i * C1_TQ;
      const int nq = min(C1_TQ, p.lout - q0);
      const int seg = (nq - 1) * p.stride + (p.k - 1) * p.dil + 1;
      const int r0 = q0 * p.stride - p.pad;
      const T* x = reinterpret_cast<const T*>(p.x) + (long)wk.seq * p.lin;
      const T* dy = reinterpret_cast<const T*>(p.dy) + ((long)wk.seq * p.lout + q0) * p.cout + c0;
      const T* ys = p.y_in ? reinterpret_cast<const T*>(p.y_in) + ((long)wk.seq * p.lout + q0) * p.cout + c0 : nullptr;
      __syncthreads();
      for (int i = threadIdx.x; i < seg; i += 256) {
        const int r = r0 + i;
        xl[i] = (r >= 0 && r < p.lin) ? lrelu_f(to_f<T>(x[r]), p.in_slope) : 0.f;
      }
      __syncthreads();
      for (int qb = ql; qb < nq; qb += ppp * UP) {
        Raw8<T> v[UP], va[UP];
#pragma unroll
        for (int u = 0; u < UP; ++u) {
          const int q = qb + u * ppp;
          if (q < nq) {
            v[u] = ld8<T>(dy + (long)q * p.cout);
            if (ys) va[u] = ld8<T>(ys + (long)q * p.cout);
          }
        }
#pragma unroll
        for (int u = 0; u < UP; ++u) {
          const int q = qb + u * ppp;
          if (q < nq) {
            float d[8], a[8];
            cvt8<T>(v[u], d);
            if (ys) {
              cvt8<T>(va[u], a);
#pragma unroll
              for (int e = 0; e < 8; ++e) d[e] *= dact_from_out(p.out_act, a[e], p.out_slope);
            }
            if (t0 == 0) {
#pragma unroll
              for (int e = 0; e < 8; ++e) bacc[e] += d[e];
            }
            const float* xr = xl + q * p.stride + t0 * p.dil;
#pragma unroll
            for (int t = 0; t < KM; ++t) {
              if (t0 + t < p.k) {
                const float xv = xr[t * p.dil];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[t][e] += d[e] * xv;
              }
            }
          }
        }
      }
      walk_add(wk, p.step_q, p.step_r, tiles);
    }
    // lanes lane % CG == cg of a wave hold partial sums of the same channels
    for (int off = CG; off < 64; off <<= 1) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        bacc[e] += __shfl_xor(bacc[e], off, 64);
#pragma unroll
        for (int t = 0; t < KM; ++t) acc[t][e] += __shfl_xor(acc[t][e], off, 64);
      }
    }
    __syncthreads();
    if (lane < CG) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[wave][cg][KM * 8 + e] = bacc[e];
#pragma unroll
        for (int t = 0; t < KM; ++t) red[wave][cg][t * 8 + e] = acc[t][e];
      }
    }
    __syncthreads();
    // scratch row = [the dW image [co][k] | cout bias sums]
    for (int i = threadIdx.x; i < (KM + 1) * p.cout; i += 256) {
      const int t = i / p.cout, co = i - t * p.cout;
      const int g = co >> 3, e = co & 7;
      const float v = ((red[0][g][t * 8 + e] + red[1][g][t * 8 + e]) + red[2][g][t * 8 + e]) + red[3][g][t * 8 + e];
      if (t < KM) {
        if (t0 + t < p.k) {
          const long idx = (long)co * p.kp + t0 + t;
          if (p.ws) p.ws[(long)blockIdx.x * p.ws_row + idx] = v;
          else atomicAdd(p.dw + idx, v);
        }
      } else if (t0 == 0) {
        if (p.ws) p.ws[(long)blockIdx.x * p.ws_row + (p.ws_row - p.cout) + co] = v;
        else if (dbias) atomicAdd(dbias + co, v);
      }
    }
  }
}

// ---- Cout == 1 backward-data: dx[i][c] = sum_t dy_eff[(i + pad - t*dil)/s] * w[t][c]; thread = 16 bytes of dx ---------
template <typename T>
__global__ __launch_bounds__(256) void cout1_bwd_data(SP p, const void* gate, const void* dx_add) {
  constexpr int V = 16 / sizeof(T);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* wl = reinterpret_cast<float*>(smem);   // [k][cin]
  const T* w = reinterpret_cast<const T*>(p.w);
  for (int i = threadIdx.x; i < p.k * p.cin; i += 256) {
    const int t = i / p.cin, c = i - t * p.cin;
    wl[i] = to_f<T>(w[sreg_index(p, 0, c, t)]);
  }
  __syncthreads();
  const int ppr = p.cin / V;
  const long total = (long)p.nseq * p.lin * ppr;
  const T* dy = reinterpret_cast<const T*>(p.dy);
  const T* ys = reinterpret_cast<const T*>(p.y_in);
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long row = idx / ppr;
    const int c0 = (int)(idx - row * ppr) * V;
    const int seq = (int)(row / p.lin), i = (int)(row - (long)seq * p.lin);
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    for (int t = 0; t < p.k; ++t) {
      const int j = i + p.pad - t * p.dil;
      if (j < 0) break;
      const int q = j / p.stride;
      if (q * p.stride != j || q >= p.lout) continue;
      const long o = (long)seq * p.lout + q;
      float d = to_f<T>(dy[o]);
      if (ys) d *= dact_from_out(p.out_act, to_f<T>(ys[o]), p.out_slope);
      const float* wr = wl + t * p.cin + c0;
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] += d * wr[e];
    }
    const long off = row * p.cin + c0;
    T outv[V];
    uint4 gv = make_uint4(0, 0, 0, 0), av = make_uint4(0, 0, 0, 0);
    if (gate) gv = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(gate) + off);
    if (dx_add) av = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(dx_add) + off);
    const T* pg = reinterpret_cast<const T*>(&gv);
    const T* pa = reinterpret_cast<const T*>(&av);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float v = acc[e];
      if (gate) v *= (to_f<T>(pg[e]) > 0.f ? 1.f : p.in_slope);
      if (dx_add) v += to_f<T>(pa[e]);
      outv[e] = from_f<T>(v);
    }
    *reinterpret_cast<uint4*>(reinterpret_cast<T*>(p.y) + off) = *reinterpret_cast<uint4*>(outv);
  }
}

SP make_sp(const evt_conv1d_params* c) {
  SP p{};
  p.nseq = c->nseq; p.lin = c->lin; p.lout = evt_conv1d_lout(c); p.cin = c->cin; p.cout = c->cout; p.k = c->k;
  p.stride = c->stride; p.pad = c->pad; p.dil = c->dil; p.in_slope = c->in_slope; p.out_act = c->out_act;
  p.out_slope = c->out_slope;
  evt_wlayout l; evt_conv1d_layout(c, &l);
  p.ck = l.reg_ck; p.nchunk = l.reg_nchunk; p.kp = l.reg_kp;
  return p;
}

inline void set_step(SP& p, long step, int len) {
  p.step_q = (int)(step / len);
  p.step_r = (int)(step - (long)p.step_q * len);
}

constexpr int CI1_WG_BLOCKS = 512;     // cin1_bwd_weight: scratch rows per weight gradient (two blocks per CU)

// ---- Cout == 1 weight gradient, x-stationary form (stride 1, dilation 1): a thread keeps ONE 16-byte piece of an input
//      row and adds it into the K taps it belongs to (output positions q = i + pad - t), so every input row is read once
//      instead of once per tap, and the per-tap dy values are 4-byte loads that hit L1.  K * V accumulators per thread.
template <typename T, int K>
__global__ __launch_bounds__(256) void cout1_bwd_weight_xs(SP p, int rows_per_block) {
  constexpr int V = 16 / sizeof(T);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* red = reinterpret_cast<float*>(smem);   // [npl][K * cin]
  const int ppr = p.cin / V;
  int pp = 1;
  while (pp < ppr) pp <<= 1;                       // pieces per row padded to a power of two (<= 256)
  const int npl = 256 / pp;                        // rows in flight per block trip
  const int rl = threadIdx.x / pp, pc = threadIdx.x % pp;
  float acc[K][V];
#pragma unroll
  for (int t = 0; t < K; ++t)
#pragma unroll
    for (int e = 0; e < V; ++e) acc[t][e] = 0.f;
  const T* x = reinterpret_cast<const T*>(p.x);
  const T* dy = reinterpret_cast<const T*>(p.dy);
  const T* ys = reinterpret_cast<const T*>(p.y_in);
  const long total = (long)p.nseq * p.lin;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(total, r0 + rows_per_block);
  constexpr int UP = 4;                            // rows per thread and trip: their loads are issued before the first use
  if (pc < ppr) {
    for (long rb = r0 + rl; rb < r1; rb += (long)npl * UP) {
      uint4 v[UP];
      float d[UP][K];
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        const long r = rb + (long)u * npl;
        const bool live = r < r1;
        const long seq = live ? r / p.lin : 0;
        const int i = live ? (int)(r - seq * p.lin) : 0;
        v[u] = live ? *reinterpret_cast<const uint4*>(x + r * p.cin + pc * V) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int t = 0; t < K; ++t) {
          const int q = i + p.pad - t;
          const bool ok = live && q >= 0 && q < p.lout;
          const long o = seq * p.lout + (ok ? q : 0);
          float dv = ok ? to_f<T>(dy[o]) : 0.f;
          if (ok && ys) dv *= dact_from_out(p.out_act, to_f<T>(ys[o]), p.out_slope);
          d[u][t] = dv;
        }
      }
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        const T* pv = reinterpret_cast<const T*>(&v[u]);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float xv = lrelu_f(to_f<T>(pv[e]), p.in_slope);
#pragma unroll
          for (int t = 0; t < K; ++t) acc[t][e] += d[u][t] * xv;
        }
      }
    }
  }
  // the row lanes of the block meet in LDS and are added in lane order (deterministic)
  const int kc = K * p.cin;
  if (pc < ppr) {
#pragma unroll
    for (int t = 0; t < K; ++t)
#pragma unroll
      for (int e = 0; e < V; ++e) red[rl * kc + t * p.cin + pc * V + e] = acc[t][e];
  }
  const long nout = (long)p.nseq * p.lout;
  const long o0 = min(nout, (long)blockIdx.x * p.pos_per_block);
  const float bsum = p.dbias ? cout1_dy_sum<T>(p, o0, min(nout, o0 + p.pos_per_block)) : 0.f;
  __syncthreads();
  cout1_store_partial(p, red, npl, bsum);
}

}  // namespace

extern "C" int evt_small_kind(const evt_conv1d_params* c) {
  if (c->transposed || c->groups != 1) return 0;
  const int V = c->dtype == EVT_DT_HALF ? 8 : 4;
  if (c->cout == 1 && c->cin % V == 0 && (long)c->k * c->cin <= 4096) return 1;   // dot-product conv
  if (c->cin == 1 && c->cout % 8 == 0 && c->cout <= 32 && 256 % c->cout == 0 && c->cout * (c->k + 1) <= 256)
    return 2;  // single-channel input
  return 0;
}

extern "C" int evt_cout1_fwd(const evt_conv1d_params* c, const void* x, const void* w_reg, const float* bias, void* y,
                             void* stream) {
  SP p = make_sp(c);
  p.x = x; p.w = w_reg; p.bias = bias; p.y = y;
  const int V = c->dtype == EVT_DT_HALF ? 8 : 4;
  const int pieces = c->k * (c->cin / V);
  int G = 1;
  while (G < pieces && G < 64) G <<= 1;
  p.G = G;
  const long total = (long)p.nseq * p.lout;
  long blocks = (total * G + 255) / 256;
  constexpr long cap = 4096;
  if (blocks > cap) blocks = cap;
  const size_t lds = (size_t)c->k * c->cin * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  evt_set_last_tag("cout1_fwd");
  if (c->dtype == EVT_DT_HALF) hipLaunchKernelGGL(cout1_fwd<h16_t>, dim3((int)blocks), dim3(256), lds, st, p);
  else hipLaunchKernelGGL(cout1_fwd<float>, dim3((int)blocks), dim3(256), lds, st, p);
  return evt_check_launch();
}

extern "C" int evt_cout1_bwd_weight(const evt_conv1d_params* c, const void* x, const void* dy, const void* y, float* dw,
                                    float* dbias, float* ws, long ws_floats, void* stream) {
  SP p = make_sp(c);
  p.x = x; p.dy = dy; p.y_in = c->out_act != EVT_ACT_NONE ? y : nullptr; p.dw = dw; p.dbias = dbias;
  const long total = (long)p.nseq * p.lout;
  long ppb = (total + 255) / 256;   // ~256 blocks: enough loads in flight, a bounded number of partial results
  if (ppb < 16) ppb = 16;
  const long img = (long)p.nchunk * p.kp * p.ck;          // d0 = 1: one row of the image
  const long row = img + 1;                               // scratch row = [image | bias sum]
  if (ws && row * 2 <= ws_floats) {
    // partial rows instead of atomics: the block count is no longer bounded by same-address atomics, and the loop is
    // latency-bound (a trip = 4 positions per lane) -- four times the blocks, a quarter of the trips
    constexpr long tgt = 1024, minp = 16;
    ppb = (total + tgt - 1) / tgt;
    if (ppb < minp) ppb = minp;
    const long maxb = ws_floats / row;
    if ((total + ppb - 1) / ppb > maxb) ppb = (total + maxb - 1) / maxb;
    p.ws = ws; p.ws_row = row;
  }
  p.pos_per_block = (int)ppb;
  int blocks = (int)((total + ppb - 1) / ppb);
  const int V = c->dtype == EVT_DT_HALF ? 8 : 4;
  hipStream_t st = (hipStream_t)stream;
  int ppr2 = 1;
  while (ppr2 < c->cin / V) ppr2 <<= 1;
  const size_t lds_xs = (size_t)(256 / ppr2) * c->k * c->cin * sizeof(float);
  if (p.stride == 1 && p.dil == 1 && (c->k == 3 || c->k == 7) && ppr2 <= 256 && lds_xs <= (60u << 10)) {
    // x-stationary form: blocks over INPUT rows (same bounds on the block count as below)
    const long rows = (long)p.nseq * p.lin;
    long rpb = (rows + blocks - 1) / blocks;
    if (rpb < 16) rpb = 16;
    blocks = (int)((rows + rpb - 1) / rpb);
    p.pos_per_block = (int)((total + blocks - 1) / blocks);   // the block's share of the outputs (bias gradient)
    evt_set_last_tag("cout1_bwd_weight_xs<k%d>", c->k);
#define XS(T, K_) hipLaunchKernelGGL((cout1_bwd_weight_xs<T, K_>), dim3(blocks), dim3(256), lds_xs, st, p, (int)rpb)
    if (c->dtype == EVT_DT_HALF) { if (c->k == 3) XS(h16_t, 3); else XS(h16_t, 7); }
    else { if (c->k == 3) XS(float, 3); else XS(float, 7); }
#undef XS
  } else {
    int pp = 1;
    while (pp < c->k * (c->cin / V) && pp < 256) pp <<= 1;
    const size_t lds = (size_t)(256 / pp) * c->k * c->cin * sizeof(float);    // one partial per position lane
    evt_set_last_tag("cout1_bwd_weight");
    if (c->dtype == EVT_DT_HALF) hipLaunchKernelGGL(cout1_bwd_weight<h16_t>, dim3(blocks), dim3(256), lds, st, p);
    else hipLaunchKernelGGL(cout1_bwd_weight<float>, dim3(blocks), dim3(256), lds, st, p);
  }
  int rc = evt_check_launch();
  if (rc || !p.ws) return rc;
  // one launch adds the rows into the image (their padded entries are written as zeros) and into the bias gradient
  return evt_conv::launch_fold_partials2(p.ws, row, blocks, dw, img, dbias, dbias ? 1 : 0, st);
}

extern "C" int evt_cin1_bwd_weight(const evt_conv1d_params* c, const void* x, const void* dy, const void* y, float* dw,
                                   float* dbias, float* ws, long ws_floats, void* stream) {
  // the Cin == 1 kernels index channel groups with masks, shuffles and a [4 waves][4 groups] LDS block: 1, 2 or 4 groups of 8
  if (c->cout != 8 && c->cout != 16 && c->cout != 32) return EVT_ENOTSUP;
  SP p = make_sp(c);
  p.x = x; p.dy = dy; p.y_in = c->out_act != EVT_ACT_NONE ? y : nullptr; p.dw = dw;
  const int tiles = (p.lout + C1_TQ - 1) / C1_TQ;
  const long ntiles = (long)p.nseq * tiles;
  // cin = 1: the image is [cout][1][kp][1] with kp == k; a scratch row holds it and the bias sums
  const long img = (long)p.cout * p.nchunk * p.kp * p.ck;
  const long row = img + p.cout;
  int blocks = (int)(ntiles < 256 ? ntiles : 256);        // atomics: <= 256 adders per dW element
  if (ws && ntiles >= 2 && row * 2 <= ws_floats) {
    const long maxb = ws_floats / row < CI1_WG_BLOCKS ? ws_floats / row : CI1_WG_BLOCKS;
    blocks = (int)(ntiles < maxb ? ntiles : maxb);
    p.ws = ws; p.ws_row = row;
  }
  set_step(p, blocks, tiles);
  const int seg = (C1_TQ - 1) * c->stride + (c->k - 1) * c->dil + 1;
  const size_t lds = (size_t)seg * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  evt_set_last_tag("cin1_bwd_weight");
#define WG(T) do { if (c->k <= 8) hipLaunchKernelGGL((cin1_bwd_weight<T, 8>), dim3(blocks), dim3(256), lds, st, p, dbias); \
                   else hipLaunchKernelGGL((cin1_bwd_weight<T, 16>), dim3(blocks), dim3(256), lds, st, p, dbias); } while (0)
  if (c->dtype == EVT_DT_HALF) WG(h16_t); else WG(float);
#undef WG
  int rc = evt_check_launch();
  if (rc || !p.ws) return rc;
  return evt_conv::launch_fold_partials2(p.ws, row, blocks, dw, img, dbias, dbias ? p.cout : 0, st);
}

extern "C" int evt_cin1_fwd(const evt_conv1d_params* c, const void* x, const void* w_reg, const float* bias, void* y,
                            void* stream) {
  SP p = make_sp(c);
  p.x = x; p.w = w_reg; p.bias = bias; p.y = y;
  const int blocks = p.nseq * ((p.lout + C1_TP - 1) / C1_TP);
  const int seg = (C1_TP - 1) * c->stride + (c->k - 1) * c->dil + 1;
  const size_t lds = ((size_t)c->k * c->cout + seg) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  evt_set_last_tag("cin1_fwd");
  if (c->dtype == EVT_DT_HALF) hipLaunchKernelGGL(cin1_fwd<h16_t>, dim3(blocks), dim3(256), lds, st, p);
  else hipLaunchKernelGGL(cin1_fwd<float>, dim3(blocks), dim3(256), lds, st, p);
  return evt_check_launch();
}

extern "C" int evt_cin1_bwd_data(const evt_conv1d_params* c, const void* dy, const void* y, const void* w_reg,
                                 const void* gate, const void* dx_add, void* dx, void* stream) {
  // the Cin == 1 kernels index channel groups with masks, shuffles and a [4 waves][4 groups] LDS block: 1, 2 or 4 groups of 8
  if (c->cout != 8 && c->cout != 16 && c->cout != 32) return EVT_ENOTSUP;
  SP p = make_sp(c);
  p.dy = dy; p.y_in = c->out_act != EVT_ACT_NONE ? y : nullptr; p.w = w_reg; p.y = dx;
  const int CG = c->cout >> 3;
  // the tile's LDS image: k tap sums per (dy row, channel group)
  int TI = C1_TI;
  size_t lds;
  for (;; TI >>= 1) {
    const int rows = (TI + (c->k - 1) * c->dil) / c->stride + 2;
    lds = ((size_t)c->k * c->cout + (size_t)rows * CG * c->k) * sizeof(float);
    if (lds <= 48 * 1024 || TI <= 32) break;
  }
  if (lds > 64 * 1024) return EVT_ENOTSUP;
  p.tile = TI;
  const int blocks = p.nseq * ((p.lin + TI - 1) / TI);
  hipStream_t st = (hipStream_t)stream;
  evt_set_last_tag("cin1_bwd_data");
#define BWD(T) do { if (c->k <= 8) hipLaunchKernelGGL((cin1_bwd_data<T, 8>), dim3(blocks), dim3(256), lds, st, p, gate, dx_add); \
                    else hipLaunchKernelGGL((cin1_bwd_data<T, 16>), dim3(blocks), dim3(256), lds, st, p, gate, dx_add); } while (0)
  if (c->dtype == EVT_DT_HALF) BWD(h16_t); else BWD(float);
#undef BWD
  return evt_check_launch();
}

extern "C" int evt_cout1_bwd_data(const evt_conv1d_params* c, const void* dy, const void* y, const void* w_reg,
                                  const void* gate, const void* dx_add, void* dx, void* stream) {
  SP p = make_sp(c);
  p.dy = dy; p.y_in = c->out_act != EVT_ACT_NONE ? y : nullptr; p.w = w_reg; p.y = dx;
  const int V = c->dtype == EVT_DT_HALF ? 8 : 4;
  const long total = (long)p.nseq * p.lin * (p.cin / V);
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  const size_t lds = (size_t)c->k * c->cin * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  evt_set_last_tag("cout1_bwd_data");
  if (c->dtype == EVT_DT_HALF) hipLaunchKernelGGL(cout1_bwd_data<h16_t>, dim3((int)blocks), dim3(256), lds, st, p, gate, dx_add);
  else hipLaunchKernelGGL(cout1_bwd_data<float>, dim3((int)blocks), dim3(256), lds, st, p, gate, dx_add);
  return evt_check_launch();
}

// Grouped strided Conv1d of DiscriminatorS (src/easevoice/module/models.py:567-570: k=41, stride 4, 4 input and
// 16 output channels per group) on MFMA, forward / backward-data / backward-weight.  gfx950 only.
//
// With cin_per_group (4) * stride (4) == 16, the im2col matrix of ONE group is a strided view of that group's
// channels-last rows laid flat in LDS:  B[k = tap*4 + c][n = q] = xs[16*q + k].  So a wave owns one group and a
// tile of positions, stages the group's rows once, and every MFMA operand is an aligned 16-byte LDS read.
// K = 41*4 = 164 is zero-padded to 192 (six 32-deep bf16 steps / 48 fp32 steps).
// Backward-data uses the same trick on dy: the 4 output phases x 4 channels form the 16 MFMA rows, and
// B[k = j*16 + co][n = q'] = dys[16*q' + k] over the 16 output channels of the group.
#include "evt_common.h"
#include "../../include/evt.h"

namespace {

template <typename T> struct GFrag;
template <> struct GFrag<float> {
  static constexpr int EPL = 1, KS = 4;
  typedef float type;
  static __device__ __forceinline__ f32x4 mma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
};
template <> struct GFrag<h16_t> {
  static constexpr int EPL = 8, KS = 32;
  typedef h16x8 type;
  static __device__ __forceinline__ f32x4 mma(h16x8 a, h16x8 b, f32x4 c) {
    return EVT_MFMA_16x16x32(a, b, c, 0, 0, 0);
  }
};
template <typename T> union GBuf;
template <> union GBuf<float> { float v; float e[1]; };
template <> union GBuf<h16_t> { h16x8 v; h16_t e[8]; };

constexpr int KPAD = 192;   // padded K (taps*4 or taps*16)
constexpr int WP = KPAD + 8;  // weight row pitch in elements (16-byte aligned, odd multiple of 16 B)
constexpr int PT = 64;      // positions per wave tile

struct GP {
  const void* x;     // fwd: x [nseq][lin][cin] ; bwd-data: dy [nseq][lout][cout]
  const void* xact;  // bwd-data: saved y (activation output) or null
  const void* w;     // REG image [cout][k][4]
  const float* bias;
  void* y;           // fwd: y ; bwd-data: dx
  float* dw;         // bwd-weight
  const void* dy;    // bwd-weight
  int nseq, lin, lout, cin, cout, k, pad, groups;
  float in_slope;
  int out_act;
  float out_slope;
  int tiles_per_seq;
  int nsplit;
  int cog;           // output channels per group: 16, or 4 (MFMA rows 4..15 are zero padding)
  const void* add;   // bwd-data: optional addend of dx (same layout), dx = T(float(T(acc)) + float(add))
  int lgp_x, lgp_dy; // 16-bit kernels: log2 of the 16-byte pieces per x row / dy row of the block's groups
};

// 16-byte staging of channels-last rows of the block's 4 groups (16 channels = 32 B bf16 / 64 B fp32 per row) into the
// per-group flat arrays gs[g][r*4 + c]; rows outside [0, nrows_total) are zeros; optional leaky-relu on load.
template <typename T>
__device__ __forceinline__ void stage_group_rows(T* gs_all, int garr, const T* src_seq, int ld, int ch0, int row0, int R,
                                                 int nrows_total, float slope) {
  constexpr int V = 16 / sizeof(T);          // channels per 16-byte piece: 8 (2 groups) or 4 (1 group)
  constexpr int PPR = 16 / V;                // pieces per row
  for (int idx = threadIdx.x; idx < R * PPR; idx += 256) {
    const int r = idx / PPR, part = idx - r * PPR;
    const int row = row0 + r;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (row >= 0 && row < nrows_total) {
      v = *reinterpret_cast<const uint4*>(src_seq + (long)row * ld + ch0 + part * V);
      if (slope != 1.f) {
        T* h = reinterpret_cast<T*>(&v);
#pragma unroll
        for (int e = 0; e < V; ++e) h[e] = from_f<T>(lrelu_f(to_f<T>(h[e]), slope));
      }
    }
    const uint2* h2 = reinterpret_cast<const uint2*>(&v);
    if constexpr (sizeof(T) == 2) {
      *reinterpret_cast<uint2*>(gs_all + (2 * part) * garr + r * 4) = h2[0];
      *reinterpret_cast<uint2*>(gs_all + (2 * part + 1) * garr + r * 4) = h2[1];
    } else {
      *reinterpret_cast<uint4*>(gs_all + part * garr + r * 4) = v;
    }
  }
}

// ---- forward: wave = one group; the block (4 groups) walks position tiles of 64 with its weights staged ONCE ----
template <typename T>
__global__ __launch_bounds__(256) void grouped_fwd(GP p) {
  constexpr int EPL = GFrag<T>::EPL, KS = GFrag<T>::KS;
  typedef typename GFrag<T>::type frag_t;
  constexpr int R = 4 * (PT - 1) + KPAD / 4;  // staged rows per tile (300)
  constexpr int GARR = R * 4 + 16;            // per-group flat array (elements)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g8 = lane >> 4;
  T* wsA = reinterpret_cast<T*>(smem) + wave * (16 * WP);
  T* xs_all = reinterpret_cast<T*>(smem) + 4 * (16 * WP);
  T* xsA = xs_all + wave * GARR;
  const int grp0 = blockIdx.y * 4;
  const int grp = grp0 + wave;
  const int K = p.k * 4;
  // stage weights of this wave's group: [16 co][K] contiguous in the REG image, zero-padded to KPAD
  const T* wg = reinterpret_cast<const T*>(p.w) + (long)grp * p.cog * K;
  for (int idx = lane; idx < 16 * KPAD; idx += 64) {
    const int co = idx / KPAD, kk = idx - co * KPAD;
    wsA[co * WP + kk] = (kk < K && co < p.cog) ? wg[co * K + kk] : from_f<T>(0.f);
  }
  float bv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bv[r] = (p.bias && g8 * 4 < p.cog) ? p.bias[grp * p.cog + g8 * 4 + r] : 0.f;
  const long total = (long)p.nseq * p.tiles_per_seq;
  for (long tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const int seq = (int)(tile / p.tiles_per_seq);
    const int q0 = (int)(tile - (long)seq * p.tiles_per_seq) * PT;
    const T* xg = reinterpret_cast<const T*>(p.x) + (long)seq * p.lin * p.cin;
    __syncthreads();     // previous tile's fragment reads are done (also orders the weight staging before first use)
    stage_group_rows<T>(xs_all, GARR, xg, p.cin, grp0 * 4, 4 * q0 - p.pad, R, p.lin, p.in_slope);
    __syncthreads();
    f32x4 acc[PT / 16];
#pragma unroll
    for (int j = 0; j < PT / 16; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int st = 0; st < KPAD / KS; ++st) {
      const int kl = st * KS + g8 * EPL;
      const frag_t a = *reinterpret_cast<const frag_t*>(wsA + n * WP + kl);
#pragma unroll
      for (int j = 0; j < PT / 16; ++j) {
        const frag_t b = *reinterpret_cast<const frag_t*>(xsA + 16 * (j * 16 + n) + kl);
        acc[j] = GFrag<T>::mma(a, b, acc[j]);
      }
    }
    T* yg = reinterpret_cast<T*>(p.y) + (long)seq * p.lout * p.cout;
#pragma unroll
    for (int j = 0; j < PT / 16; ++j) {
      const int q = q0 + j * 16 + n;
      if (q >= p.lout || g8 * 4 >= p.cog) continue;
      const int co = grp * p.cog + g8 * 4;
      T outv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[j][r] + bv[r];
        if (p.out_act == EVT_ACT_LRELU) v = lrelu_f(v, p.out_slope);
        else if (p.out_act == EVT_ACT_TANH) v = tanhf(v);
        outv[r] = from_f<T>(v);
      }
      T* dst = yg + (long)q * p.cout + co;
      if constexpr (sizeof(T) == 2) *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<uint2*>(outv);
      else *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<uint4*>(outv);
    }
  }
}

// 16-byte staging of dy rows (the block's 4 groups = 4*cog contiguous channels) into per-group arrays gs[g][r*16 + co],
// times act'(y) when `ya` is given; slots co >= cog stay zero (the arrays are cleared once per block).
template <typename T>
__device__ __forceinline__ void stage_dy_rows(T* gs_all, int garr, const T* dy_seq, const T* ya_seq, int ld, int ch0, int cog,
                                              int row0, int R, int nrows_total, int act, float slope) {
  constexpr int V = 16 / sizeof(T);
  const int ppr = 4 * cog / V;               // pieces per row (cog in {4, 16}: 2/8 bf16, 4/16 fp32)
  for (int idx = threadIdx.x; idx < R * ppr; idx += 256) {
    const int r = idx / ppr, part = idx - r * ppr;
    const int row = row0 + r;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (row >= 0 && row < nrows_total) {
      const long off = (long)row * ld + ch0 + part * V;
      v = *reinterpret_cast<const uint4*>(dy_seq + off);
      if (ya_seq) {
        const uint4 va = *reinterpret_cast<const uint4*>(ya_seq + off);
        T* h = reinterpret_cast<T*>(&v);
        const T* ha = reinterpret_cast<const T*>(&va);
#pragma unroll
        for (int e = 0; e < V; ++e) h[e] = from_f<T>(to_f<T>(h[e]) * dact_from_out(act, to_f<T>(ha[e]), slope));
      }
    }
    const int c = part * V;                  // first channel of the piece inside the block's 4*cog channels
    if (cog >= V) {
      *reinterpret_cast<uint4*>(gs_all + (c / cog) * garr + r * 16 + (c % cog)) = v;
    } else {                                 // bf16, cog = 4: the piece holds two groups of 4 channels
      const uint2* h2 = reinterpret_cast<const uint2*>(&v);
      *reinterpret_cast<uint2*>(gs_all + (c / cog) * garr + r * 16) = h2[0];
      *reinterpret_cast<uint2*>(gs_all + (c / cog + 1) * garr + r * 16) = h2[1];
    }
  }
}

// ---- backward-data: wave = one group, rows 4q' + phase - pad, 16 MFMA rows = (phase, c); persistent over q' tiles ----
template <typename T>
__global__ __launch_bounds__(256) void grouped_bwd_data(GP p) {
  constexpr int EPL = GFrag<T>::EPL, KS = GFrag<T>::KS;
  typedef typename GFrag<T>::type frag_t;
  constexpr int JP = KPAD / 16;            // 12 padded "j" taps of 16 output channels
  constexpr int R = PT + JP - 1;           // staged dy rows per tile
  constexpr int GARR = R * 16 + 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g8 = lane >> 4;
  T* wsA = reinterpret_cast<T*>(smem) + wave * (16 * WP);
  T* ds_all = reinterpret_cast<T*>(smem) + 4 * (16 * WP);
  T* dsA = ds_all + wave * GARR;
  const int grp0 = blockIdx.y * 4;
  const int grp = grp0 + wave;
  const int K = p.k * 4;
  // A[(phase, c)][(jj, co)] = w[grp*16+co][t = phase + 4*(JP-1-jj)][c], zero when t >= k
  const T* wg = reinterpret_cast<const T*>(p.w) + (long)grp * p.cog * K;
  for (int idx = lane; idx < 16 * KPAD; idx += 64) {
    const int m = idx / KPAD, kk = idx - m * KPAD;
    const int ph = m >> 2, c = m & 3;
    const int jj = kk >> 4, co = kk & 15;
    const int t = ph + 4 * (JP - 1 - jj);
    wsA[m * WP + kk] = (t < p.k && co < p.cog) ? wg[co * K + t * 4 + c] : from_f<T>(0.f);
  }
  for (int idx = tid; idx < 4 * GARR; idx += 256) ds_all[idx] = from_f<T>(0.f);
  const long total = (long)p.nseq * p.tiles_per_seq;
  for (long tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const int seq = (int)(tile / p.tiles_per_seq);
    const int q0 = (int)(tile - (long)seq * p.tiles_per_seq) * PT;   // first q' of the tile
    const T* dyg = reinterpret_cast<const T*>(p.x) + (long)seq * p.lout * p.cout;
    const T* yag = p.xact ? reinterpret_cast<const T*>(p.xact) + (long)seq * p.lout * p.cout : nullptr;
    __syncthreads();
    stage_dy_rows<T>(ds_all, GARR, dyg, yag, p.cout, grp0 * p.cog, p.cog, q0 - (JP - 1), R, p.lout, p.out_act, p.out_slope);
    __syncthreads();
    f32x4 acc[PT / 16];
#pragma unroll
    for (int j = 0; j < PT / 16; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int st = 0; st < KPAD / KS; ++st) {
      const int kl = st * KS + g8 * EPL;
      const frag_t a = *reinterpret_cast<const frag_t*>(wsA + n * WP + kl);
#pragma unroll
      for (int j = 0; j < PT / 16; ++j) {
        const frag_t b = *reinterpret_cast<const frag_t*>(dsA + 16 * (j * 16 + n) + kl);
        acc[j] = GFrag<T>::mma(a, b, acc[j]);
      }
    }
    // lane holds MFMA rows g8*4 + r = (phase g8, channel r) of column q'
    T* dxg = reinterpret_cast<T*>(p.y) + (long)seq * p.lin * p.cin;
#pragma unroll
    for (int j = 0; j < PT / 16; ++j) {
      const int qp = q0 + j * 16 + n;
      const int row = 4 * qp + g8 - p.pad;
      if (row < 0 || row >= p.lin) continue;
      T outv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) outv[r] = from_f<T>(acc[j][r]);
      if (p.add) {                             // rounds to storage first, as a separate add would
        const T* ad = reinterpret_cast<const T*>(p.add) + (long)seq * p.lin * p.cin + (long)row * p.cin + grp * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) outv[r] = from_f<T>(to_f<T>(outv[r]) + to_f<T>(ad[r]));
      }
      T* dst = dxg + (long)row * p.cin + grp * 4;
      if constexpr (sizeof(T) == 2) *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<uint2*>(outv);
      else *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<uint4*>(outv);
    }
  }
}

// ---- backward-weight: wave = group; blocks split the positions; dW[co][t*4+c] += dy[q][co] * x[16q + t*4 + c] ----
template <typename T>
__global__ __launch_bounds__(256) void grouped_bwd_weight(GP p) {
  constexpr int EPL = GFrag<T>::EPL, KS = GFrag<T>::KS;
  typedef typename GFrag<T>::type frag_t;
  constexpr int NTB = 11;                     // 11 tiles of 16 cover K = 164 (176)
  constexpr int R = 4 * (PT - 1) + 44;        // rows touched by 64 positions x 44 (padded) taps
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g8 = lane >> 4;
  T* dsA = reinterpret_cast<T*>(smem) + wave * (PT * 16 + R * 4 + 32);
  T* xsA = dsA + PT * 16 + 16;
  const int grp = blockIdx.y * 4 + wave;
  const int K = p.k * 4;
  const T* xg0 = reinterpret_cast<const T*>(p.x);
  const T* dy0 = reinterpret_cast<const T*>(p.dy);
  const T* ya0 = reinterpret_cast<const T*>(p.xact);
  f32x4 acc[NTB];
#pragma unroll
  for (int j = 0; j < NTB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const long total = (long)p.nseq * p.tiles_per_seq;
  for (long it = blockIdx.x; it < total; it += p.nsplit) {
    const int seq = (int)(it / p.tiles_per_seq);
    const int q0 = (int)(it % p.tiles_per_seq) * PT;
    __syncthreads();
    for (int idx = lane; idx < PT * 16; idx += 64) {
      const int r = idx >> 4, co = idx & 15;
      const int q = q0 + r;
      T v = from_f<T>(0.f);
      if (q < p.lout && co < p.cog) {
        const long off = ((long)seq * p.lout + q) * p.cout + grp * p.cog + co;
        float f = to_f<T>(dy0[off]);
        if (ya0) f *= dact_from_out(p.out_act, to_f<T>(ya0[off]), p.out_slope);
        v = from_f<T>(f);
      }
      dsA[r * 16 + co] = v;
    }
    const int row0 = 4 * q0 - p.pad;
    for (int idx = lane; idx < R * 4; idx += 64) {
      const int r = idx >> 2, c = idx & 3;
      const int row = row0 + r;
      T v = from_f<T>(0.f);
      if (row >= 0 && row < p.lin)
        v = from_f<T>(lrelu_f(to_f<T>(xg0[((long)seq * p.lin + row) * p.cin + grp * 4 + c]), p.in_slope));
      xsA[r * 4 + c] = v;
    }
    __syncthreads();
#pragma unroll 1
    for (int kk = 0; kk < PT / KS; ++kk) {
      const int k0 = kk * KS + g8 * EPL;
      GBuf<T> av;
#pragma unroll
      for (int e = 0; e < EPL; ++e) av.e[e] = dsA[(k0 + e) * 16 + n];
      const frag_t a = av.v;
#pragma unroll
      for (int j = 0; j < NTB; ++j) {
        GBuf<T> bv;
#pragma unroll
        for (int e = 0; e < EPL; ++e) bv.e[e] = xsA[16 * (k0 + e) + j * 16 + n];
        acc[j] = GFrag<T>::mma(a, bv.v, acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NTB; ++j) {
    const int kidx = j * 16 + n;
    if (kidx >= K) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (g8 * 4 + r >= p.cog) continue;
      const int co = grp * p.cog + g8 * 4 + r;
      atomicAdd(p.dw + (long)co * K + kidx, acc[j][r]);
    }
  }
}

// ================= 16-bit kernels: weights in registers, register-prefetched tiles, wide rows =======================
// Same GEMMs and the same LDS views as the templates above (which now serve fp32 only); what differs is the schedule.
//  * A block owns GB groups, one per wave (blockDim = 64 * GB).  GB = 16 where the group count allows it, so a block
//    reads 128 contiguous bytes of every x row and writes 512 (cog 16) / 128 (cog 4) of every y row.
//  * The A operand depends only on (lane, K step): six 16-byte fragments = 24 VGPRs, loaded once per block straight
//    from the REG image (forward: two 8-byte loads per fragment).  No weight staging in LDS.
//  * While a tile's MFMAs and stores run, the rows of the block's next tile are in flight into registers (unconditional
//    loads from clamped addresses; a plain __syncthreads() does not drain them).  They go to LDS after the barrier that
//    retires the current tile's fragment reads.
//  * A partial last tile computes and stages only its 16-position sub-tiles (lout 80 = 64 + 16: the second tile does a
//    quarter of the work).
// The K steps of every output element keep their order (six 32-deep steps, taps in image order), so y and dx have the
// bits the previous kernels gave.

// smallest per-group LDS pitch (elements) >= `elems` whose dword count is `m` modulo `mod` (spreads the staging writes
// of neighbouring groups over the banks)
constexpr int lds_pitch(int elems, int m, int mod) {
  int p = (elems + 1) / 2;
  while (p % mod != m) ++p;
  return 2 * p;
}

// this thread's 16-byte pieces (threadIdx.x + i * blockDim.x) of rows [row0, row0 + R) x (8 << lgp) channels from ch0.
// Rows outside [0, nrows_total) and pieces past row R read as zeros.
template <int NP>
__device__ __forceinline__ void pre_load(uint4 (&v)[NP], const h16_t* src_seq, int ld, int ch0, int row0, int R,
                                         int nrows_total, int lgp) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int idx = threadIdx.x + i * blockDim.x;
    const int r = idx >> lgp, part = idx & ((1 << lgp) - 1);
    const int row = row0 + r;
    const bool ok = r < R && row >= 0 && row < nrows_total;
    const uint4 t = *reinterpret_cast<const uint4*>(src_seq + (long)(ok ? row : 0) * ld + ch0 + part * 8);
    v[i] = ok ? t : make_uint4(0, 0, 0, 0);
  }
}

// prefetched x pieces -> per-group flat arrays gs[g][r*4 + c] (leaky-relu on the way)
template <int NP>
__device__ __forceinline__ void put_x(h16_t* gs_all, int garr, const uint4 (&v)[NP], int R, int lgp, float slope) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int idx = threadIdx.x + i * blockDim.x;
    const int r = idx >> lgp, part = idx & ((1 << lgp) - 1);
    if (r >= R) continue;
    uint4 t = v[i];
    if (slope != 1.f) {
      h16_t* h = reinterpret_cast<h16_t*>(&t);
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = from_f<h16_t>(lrelu_f(to_f<h16_t>(h[e]), slope));
    }
    const uint2* h2 = reinterpret_cast<const uint2*>(&t);
    *reinterpret_cast<uint2*>(gs_all + (2 * part) * garr + r * 4) = h2[0];
    *reinterpret_cast<uint2*>(gs_all + (2 * part + 1) * garr + r * 4) = h2[1];
  }
}

// prefetched dy (and y) pieces -> per-group arrays gs[g][r*16 + co], times act'(y); slots co >= cog are never written
template <int NP>
__device__ __forceinline__ void put_dy(h16_t* gs_all, int garr, const uint4 (&v)[NP], const uint4 (&va)[NP], bool has_ya,
                                       int cog, int R, int lgp, int act, float slope) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int idx = threadIdx.x + i * blockDim.x;
    const int r = idx >> lgp, part = idx & ((1 << lgp) - 1);
    if (r >= R) continue;
    uint4 t = v[i];
    if (has_ya) {
      const uint4 ta = va[i];
      h16_t* h = reinterpret_cast<h16_t*>(&t);
      const h16_t* ha = reinterpret_cast<const h16_t*>(&ta);
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = from_f<h16_t>(to_f<h16_t>(h[e]) * dact_from_out(act, to_f<h16_t>(ha[e]), slope));
    }
    const int c = part * 8;                    // first channel of the piece inside the block's GB*cog channels
    if (cog >= 8) {
      *reinterpret_cast<uint4*>(gs_all + (c / cog) * garr + r * 16 + (c % cog)) = t;
    } else {                                   // cog = 4: the piece holds two groups of 4 channels
      const uint2* h2 = reinterpret_cast<const uint2*>(&t);
      *reinterpret_cast<uint2*>(gs_all + (c / cog) * garr + r * 16) = h2[0];
      *reinterpret_cast<uint2*>(gs_all + (c / cog + 1) * garr + r * 16) = h2[1];
    }
  }
}

constexpr int F_R = 4 * (PT - 1) + KPAD / 4;        // forward: staged x rows of a full tile (300)
constexpr int F_GARR = lds_pitch(F_R * 4, 8, 32);   // 1232: neighbouring group pairs land 16 banks apart
constexpr int F_NP = (F_R + 127) / 128;             // pieces per thread: F_R * GB/2 pieces over 64 * GB threads

// ---- forward ----
__global__ __launch_bounds__(1024) void grouped_fwd16(GP p) {
  typedef h16_t T;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g8 = lane >> 4;
  T* xs_all = reinterpret_cast<T*>(smem);
  const T* xsA = xs_all + wave * F_GARR;
  const int GB = blockDim.x >> 6;
  const int grp0 = blockIdx.y * GB, grp = grp0 + wave;
  const int K = p.k * 4;
  // A[co = n][k = st*32 + g8*8 ..+8]: rows of the REG image [cout][k][4] are K = 4k elements (8-byte aligned pieces)
  h16x8 a[KPAD / 32];
  {
    const bool rok = n < p.cog;
    const T* wrow = reinterpret_cast<const T*>(p.w) + ((long)grp * p.cog + (rok ? n : 0)) * K;
#pragma unroll
    for (int st = 0; st < KPAD / 32; ++st) {
      const int kl = st * 32 + g8 * 8;
      const bool ok0 = rok && kl < K, ok1 = rok && kl + 4 < K;
      const uint2 lo = *reinterpret_cast<const uint2*>(wrow + (ok0 ? kl : 0));
      const uint2 hi = *reinterpret_cast<const uint2*>(wrow + (ok1 ? kl + 4 : 0));
      union { uint4 u; h16x8 v; } f;
      f.u = make_uint4(ok0 ? lo.x : 0u, ok0 ? lo.y : 0u, ok1 ? hi.x : 0u, ok1 ? hi.y : 0u);
      a[st] = f.v;
    }
  }
  float bv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bv[r] = (p.bias && g8 * 4 < p.cog) ? p.bias[grp * p.cog + g8 * 4 + r] : 0.f;
  const T* x0 = reinterpret_cast<const T*>(p.x);
  const long total = (long)p.nseq * p.tiles_per_seq;
  int seq = 0, q0 = 0, nj = 0;                 // geometry of the tile in `pre`
  auto locate = [&](long t) {
    seq = (int)(t / p.tiles_per_seq);
    q0 = (int)(t - (long)seq * p.tiles_per_seq) * PT;
    const int left = p.lout - q0;
    nj = left >= PT ? PT / 16 : (left + 15) >> 4;
  };
  uint4 pre[F_NP];
  long tile = blockIdx.x;
  if (tile < total) {
    locate(tile);
    pre_load<F_NP>(pre, x0 + (long)seq * p.lin * p.cin, p.cin, grp0 * 4, 4 * q0 - p.pad, 64 * nj + 44, p.lin, p.lgp_x);
  }
  for (; tile < total; tile += gridDim.x) {
    const int cseq = seq, cq0 = q0, cnj = nj;
    __syncthreads();                           // the previous tile's fragment reads are done
    put_x<F_NP>(xs_all, F_GARR, pre, 64 * cnj + 44, p.lgp_x, p.in_slope);
    __syncthreads();
    if (tile + gridDim.x < total) {            // next tile's rows fly during the MFMAs and stores below
      locate(tile + gridDim.x);
      pre_load<F_NP>(pre, x0 + (long)seq * p.lin * p.cin, p.cin, grp0 * 4, 4 * q0 - p.pad, 64 * nj + 44, p.lin, p.lgp_x);
    }
    T* yg = reinterpret_cast<T*>(p.y) + (long)cseq * p.lout * p.cout;
#pragma unroll
    for (int j = 0; j < PT / 16; ++j) {
      if (j >= cnj) break;
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < KPAD / 32; ++st) {
        const h16x8 b = *reinterpret_cast<const h16x8*>(xsA + 16 * (j * 16 + n) + st * 32 + g8 * 8);
        acc = EVT_MFMA_16x16x32(a[st], b, acc, 0, 0, 0);
      }
      const int q = cq0 + j * 16 + n;
      if (q >= p.lout || g8 * 4 >= p.cog) continue;
      T outv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[r] + bv[r];
        if (p.out_act == EVT_ACT_LRELU) v = lrelu_f(v, p.out_slope);
        else if (p.out_act == EVT_ACT_TANH) v = tanhf(v);
        outv[r] = from_f<T>(v);
      }
      *reinterpret_cast<uint2*>(yg + (long)q * p.cout + grp * p.cog + g8 * 4) = *reinterpret_cast<uint2*>(outv);
    }
  }
}

constexpr int D_JP = KPAD / 16;                     // 12 padded "j" taps of 16 output channels
constexpr int D_R = PT + D_JP - 1;                  // backward-data: staged dy rows of a full tile (75)
constexpr int D_GARR = lds_pitch(D_R * 16, 8, 64);  // 1296: the 16-byte pieces of 8 neighbouring groups tile the banks
constexpr int D_NP = (D_R * 16 + 511) / 512;        // pieces per thread: D_R * GB*cog/8 pieces over 64 * GB threads, cog <= 16

// ---- backward-data: 16 MFMA rows = (phase, c), columns q'; dx row = 4q' + phase - pad ----
__global__ __launch_bounds__(1024) void grouped_bwd_data16(GP p) {
  typedef h16_t T;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g8 = lane >> 4;
  T* ds_all = reinterpret_cast<T*>(smem);
  const T* dsA = ds_all + wave * D_GARR;
  const int GB = blockDim.x >> 6;
  const int grp0 = blockIdx.y * GB, grp = grp0 + wave;
  const int K = p.k * 4;
  // A[(phase, c) = n][(jj, co)] = w[grp*cog + co][t = phase + 4*(JP-1-jj)][c], zero when t >= k: a gather over the
  // rows of the image, 48 two-byte loads per lane, once per block
  h16x8 a[KPAD / 32];
  {
    const T* wg = reinterpret_cast<const T*>(p.w) + (long)grp * p.cog * K;
    const int ph = n >> 2, c = n & 3;
#pragma unroll
    for (int st = 0; st < KPAD / 32; ++st) {
      const int t = ph + 4 * (D_JP - 1 - (st * 2 + (g8 >> 1)));
      union { h16_t e[8]; h16x8 v; } f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int co = (g8 & 1) * 8 + e;
        const bool ok = t < p.k && co < p.cog;
        const T w = wg[ok ? co * K + t * 4 + c : 0];
        f.e[e] = ok ? w : (T)0;
      }
      a[st] = f.v;
    }
  }
  for (int idx = tid; idx < GB * D_GARR; idx += blockDim.x) ds_all[idx] = (T)0;
  const T* dy0 = reinterpret_cast<const T*>(p.x);
  const T* ya0 = reinterpret_cast<const T*>(p.xact);
  const T* ad0 = reinterpret_cast<const T*>(p.add);
  const bool has_ya = ya0 != nullptr;
  const long total = (long)p.nseq * p.tiles_per_seq;
  int seq = 0, q0 = 0, nj = 0;
  auto locate = [&](long t) {
    seq = (int)(t / p.tiles_per_seq);
    q0 = (int)(t - (long)seq * p.tiles_per_seq) * PT;   // first q' of the tile
    const int left = p.nsplit - q0;                     // nsplit carries the number of q' per sequence
    nj = left >= PT ? PT / 16 : (left + 15) >> 4;
  };
  uint4 pre[D_NP], prea[D_NP];
#pragma unroll
  for (int i = 0; i < D_NP; ++i) prea[i] = make_uint4(0, 0, 0, 0);
  auto fetch = [&]() {
    const long so = (long)seq * p.lout * p.cout;
    pre_load<D_NP>(pre, dy0 + so, p.cout, grp0 * p.cog, q0 - (D_JP - 1), 16 * nj + D_JP - 1, p.lout, p.lgp_dy);
    if (has_ya) pre_load<D_NP>(prea, ya0 + so, p.cout, grp0 * p.cog, q0 - (D_JP - 1), 16 * nj + D_JP - 1, p.lout, p.lgp_dy);
  };
  long tile = blockIdx.x;
  if (tile < total) {
    locate(tile);
    fetch();
  }
  for (; tile < total; tile += gridDim.x) {
    const int cseq = seq, cq0 = q0, cnj = nj;
    __syncthreads();
    put_dy<D_NP>(ds_all, D_GARR, pre, prea, has_ya, p.cog, 16 * cnj + D_JP - 1, p.lgp_dy, p.out_act, p.out_slope);
    __syncthreads();
    if (tile + gridDim.x < total) {
      locate(tile + gridDim.x);
      fetch();
    }
    // lane holds MFMA rows g8*4 + r = (phase g8, channel r) of column q'
    const long xo = (long)cseq * p.lin * p.cin + grp * 4;
    T* dxg = reinterpret_cast<T*>(p.y) + xo;
    uint2 av[PT / 16];
    if (ad0) {
#pragma unroll
      for (int j = 0; j < PT / 16; ++j) {
        const int row = 4 * (cq0 + j * 16 + n) + g8 - p.pad;
        const bool ok = row >= 0 && row < p.lin;
        av[j] = *reinterpret_cast<const uint2*>(ad0 + xo + (long)(ok ? row : 0) * p.cin);
      }
    }
#pragma unroll
    for (int j = 0; j < PT / 16; ++j) {
      if (j >= cnj) break;
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < KPAD / 32; ++st) {
        const h16x8 b = *reinterpret_cast<const h16x8*>(dsA + 16 * (j * 16 + n) + st * 32 + g8 * 8);
        acc = EVT_MFMA_16x16x32(a[st], b, acc, 0, 0, 0);
      }
      const int row = 4 * (cq0 + j * 16 + n) + g8 - p.pad;
      if (row < 0 || row >= p.lin) continue;
      T outv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) outv[r] = from_f<T>(acc[r]);
      if (ad0) {                                 // rounds to storage first, as the separate add did
        const T* ah = reinterpret_cast<const T*>(&av[j]);
#pragma unroll
        for (int r = 0; r < 4; ++r) outv[r] = from_f<T>(to_f<T>(outv[r]) + to_f<T>(ah[r]));
      }
      *reinterpret_cast<uint2*>(dxg + (long)row * p.cin) = *reinterpret_cast<uint2*>(outv);
    }
  }
}

// ---- backward-weight: vector staging + transpose-read fragments ---------------------------------------------------
// GEMM of the fp32 kernel above (M = the group's 16 output channels, N = (tap, c) = 11 tiles of 16, K = positions).
// dy is staged position-major for the block's 4 groups, x as the flat per-group row array of the forward kernel, and
// BOTH MFMA operands -- 8 consecutive positions of one column -- come from ds_read_b64_tr_b16: the row address is per
// lane, so the overlapping-window view B[pos][kidx] = xs[16*pos + kidx] is just an address.  All 24 transpose reads of
// a 32-position step are issued back to back behind ONE wait (tile j of B is the immediate offset 32*j bytes).
// The block stays at 4 groups: every block adds its whole 4 x 16 x 164 slice to dW with fp32 atomics, which execute at
// the memory side, so their number (slice x blocks) is kept down rather than the rows widened.
#define EVT_TR(o, b, off) "ds_read_b64_tr_b16 %" #o ", %" #b " offset:" #off "\n\t"
__device__ __forceinline__ void g_tr_step(const h16_t* pa, const h16_t* pb, h16x8& a, h16x8 (&b)[11]) {
  const unsigned aa = (unsigned)(uintptr_t)pa, ab = (unsigned)(uintptr_t)pb;
  uint2 r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15, r16, r17, r18, r19, r20, r21, r22, r23;
  asm volatile(
      EVT_TR(0, 24, 0) EVT_TR(1, 24, 128)
      EVT_TR(2, 25, 0) EVT_TR(3, 25, 128) EVT_TR(4, 25, 32) EVT_TR(5, 25, 160)
      EVT_TR(6, 25, 64) EVT_TR(7, 25, 192) EVT_TR(8, 25, 96) EVT_TR(9, 25, 224)
      EVT_TR(10, 25, 128) EVT_TR(11, 25, 256) EVT_TR(12, 25, 160) EVT_TR(13, 25, 288)
      EVT_TR(14, 25, 192) EVT_TR(15, 25, 320) EVT_TR(16, 25, 224) EVT_TR(17, 25, 352)
      EVT_TR(18, 25, 256) EVT_TR(19, 25, 384) EVT_TR(20, 25, 288) EVT_TR(21, 25, 416)
      EVT_TR(22, 25, 320) EVT_TR(23, 25, 448)
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7), "=&v"(r8), "=&v"(r9),
        "=&v"(r10), "=&v"(r11), "=&v"(r12), "=&v"(r13), "=&v"(r14), "=&v"(r15), "=&v"(r16), "=&v"(r17), "=&v"(r18),
        "=&v"(r19), "=&v"(r20), "=&v"(r21), "=&v"(r22), "=&v"(r23)
      : "v"(aa), "v"(ab)
      : "memory");
  union { uint4 u; h16x8 v; } f;
#define EVT_FR(lo, hi) (f.u = make_uint4(lo.x, lo.y, hi.x, hi.y), f.v)
  a = EVT_FR(r0, r1);
  b[0] = EVT_FR(r2, r3); b[1] = EVT_FR(r4, r5); b[2] = EVT_FR(r6, r7); b[3] = EVT_FR(r8, r9);
  b[4] = EVT_FR(r10, r11); b[5] = EVT_FR(r12, r13); b[6] = EVT_FR(r14, r15); b[7] = EVT_FR(r16, r17);
  b[8] = EVT_FR(r18, r19); b[9] = EVT_FR(r20, r21); b[10] = EVT_FR(r22, r23);
#undef EVT_FR
}
#undef EVT_TR

constexpr int W_NTB = 11;                     // 11 tiles of 16 cover K = 164 (176)
constexpr int W_R = 4 * (PT - 1) + 44;        // rows touched by 64 positions x 44 (padded) taps
constexpr int W_GARR = W_R * 4 + 32;          // flat per-group x array (+ slack for the padded taps of the last rows)
constexpr int W_DARR = PT * 16;               // per-group dy tile [pos][16]
constexpr int W_NPX = (W_R * 2 + 255) / 256;  // x pieces per thread (2 per row, 256 threads)
constexpr int W_NPD = (PT * 8 + 255) / 256;   // dy pieces per thread (at most 8 per row)

__global__ __launch_bounds__(256) void grouped_bwd_weight_tr(GP p) {
  typedef h16_t T;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g8 = lane >> 4;
  T* ds_all = reinterpret_cast<T*>(smem);
  T* xs_all = ds_all + 4 * W_DARR;
  const T* dsA = ds_all + wave * W_DARR;
  const T* xsA = xs_all + wave * W_GARR;
  const int grp0 = blockIdx.y * 4, grp = grp0 + wave;
  const int K = p.k * 4;
  for (int idx = tid; idx < 4 * W_DARR + 4 * W_GARR; idx += 256) ds_all[idx] = (T)0;
  f32x4 acc[W_NTB];
#pragma unroll
  for (int j = 0; j < W_NTB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const T* x0 = reinterpret_cast<const T*>(p.x);
  const T* dy0 = reinterpret_cast<const T*>(p.dy);
  const T* ya0 = reinterpret_cast<const T*>(p.xact);
  const bool has_ya = ya0 != nullptr;
  const long total = (long)p.nseq * p.tiles_per_seq;
  int seq = 0, q0 = 0, nk = 0;                 // nk: 32-position steps of the tile that hold positions
  auto locate = [&](long t) {
    seq = (int)(t / p.tiles_per_seq);
    q0 = (int)(t - (long)seq * p.tiles_per_seq) * PT;
    const int left = p.lout - q0;
    nk = left >= PT ? PT / 32 : (left + 31) >> 5;
  };
  uint4 px[W_NPX], pd[W_NPD], pa[W_NPD];
#pragma unroll
  for (int i = 0; i < W_NPD; ++i) pa[i] = make_uint4(0, 0, 0, 0);
  auto fetch = [&]() {
    const long so = (long)seq * p.lout * p.cout;
    pre_load<W_NPD>(pd, dy0 + so, p.cout, grp0 * p.cog, q0, 32 * nk, p.lout, p.lgp_dy);
    if (has_ya) pre_load<W_NPD>(pa, ya0 + so, p.cout, grp0 * p.cog, q0, 32 * nk, p.lout, p.lgp_dy);
    pre_load<W_NPX>(px, x0 + (long)seq * p.lin * p.cin, p.cin, grp0 * 4, 4 * q0 - p.pad, 128 * nk + 40, p.lin, 1);
  };
  long it = blockIdx.x;
  if (it < total) {
    locate(it);
    fetch();
  }
  for (; it < total; it += p.nsplit) {
    const int cnk = nk;
    __syncthreads();
    put_dy<W_NPD>(ds_all, W_DARR, pd, pa, has_ya, p.cog, 32 * cnk, p.lgp_dy, p.out_act, p.out_slope);
    put_x<W_NPX>(xs_all, W_GARR, px, 128 * cnk + 40, 1, p.in_slope);
    __syncthreads();
    if (it + p.nsplit < total) {
      locate(it + p.nsplit);
      fetch();
    }
#pragma unroll
    for (int kk = 0; kk < PT / 32; ++kk) {
      if (kk >= cnk) break;
      const int kb = kk * 32 + g8 * 8;        // first of this lane group's 8 positions
      h16x8 a, b[W_NTB];
      g_tr_step(dsA + (kb + (n >> 2)) * 16 + 4 * (n & 3), xsA + 16 * (kb + (n >> 2)) + 4 * (n & 3), a, b);
#pragma unroll
      for (int j = 0; j < W_NTB; ++j) acc[j] = EVT_MFMA_16x16x32(a, b[j], acc[j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < W_NTB; ++j) {
    const int kidx = j * 16 + n;
    if (kidx >= K) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (g8 * 4 + r >= p.cog) continue;
      const int co = grp * p.cog + g8 * 4 + r;
      atomicAdd(p.dw + (long)co * K + kidx, acc[j][r]);
    }
  }
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// compute units of the current device (grids are sized by the chip)
inline int chip_cus() {
  static int n = 0;
  if (n <= 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
    if (n <= 0) n = 256;
  }
  return n;
}

// blocks along x of the persistent fp32 forward / backward-data kernels: ~3 blocks per CU over all group sets, each
// block amortises its weight staging (3072 elements per wave) over several position tiles
inline int persistent_blocks(long tiles, int group_sets) {
  long b = (3 * chip_cus() + group_sets - 1) / group_sets;
  if (b > tiles) b = tiles;
  if (b < 1) b = 1;
  return (int)b;
}

// 16-bit kernels: groups per block (one wave each) -- 16 where the group count allows it
inline int groups_per_block(int groups) { return groups % 16 == 0 ? 16 : groups % 8 == 0 ? 8 : 4; }
inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// 16-bit forward / backward-data: blocks along x.  G16_WAVES_PER_CU waves on every CU over all group sets, in blocks of
// gb waves: one 16-wave block or four 4-wave blocks per CU (74 / 105 VGPRs: 6 / 4 waves per SIMD fit).
constexpr int G16_WAVES_PER_CU = 16;
inline int blocks16(long tiles, int gb, int group_sets) {
  long b = (long)chip_cus() * G16_WAVES_PER_CU / ((long)gb * group_sets);
  if (b > tiles) b = tiles;
  if (b < 1) b = 1;
  return (int)b;
}

template <typename F>
int set_lds(F f, size_t lds) {
  if (lds > 48 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(f), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess)
      return EVT_ELAUNCH;
  }
  return EVT_OK;
}

}  // namespace

// Shape gate shared with conv1d.hip's dispatcher.
extern "C" int evt_grouped_supported(const evt_conv1d_params* c) {
  return !c->transposed && c->groups > 1 && c->groups % 4 == 0 && c->cin / c->groups == 4 && (c->cout / c->groups == 16 || c->cout / c->groups == 4) &&
         c->stride == 4 && c->dil == 1 && c->k * 4 <= 176 && c->k >= 4;
}

extern "C" int evt_grouped_fwd(const evt_conv1d_params* c, const void* x, const void* w_reg, const float* bias, void* y,
                               void* stream) {
  GP p{};
  p.x = x; p.w = w_reg; p.bias = bias; p.y = y;
  p.nseq = c->nseq; p.lin = c->lin; p.lout = evt_conv1d_lout(c); p.cin = c->cin; p.cout = c->cout; p.k = c->k;
  p.pad = c->pad; p.groups = c->groups; p.in_slope = c->in_slope; p.out_act = c->out_act; p.out_slope = c->out_slope;
  p.cog = c->cout / c->groups;
  p.tiles_per_seq = cdiv(p.lout, PT);
  hipStream_t st = (hipStream_t)stream;
  if (c->dtype == EVT_DT_HALF) {
    const int gb = groups_per_block(c->groups);
    p.lgp_x = ilog2(gb / 2); p.lgp_dy = ilog2(gb * p.cog / 8);
    const size_t lds = (size_t)gb * F_GARR * 2;
    dim3 grid(blocks16((long)p.nseq * p.tiles_per_seq, gb, c->groups / gb), c->groups / gb);
    if (set_lds(&grouped_fwd16, lds)) return EVT_ELAUNCH;
    hipLaunchKernelGGL(grouped_fwd16, grid, dim3(64 * gb), lds, st, p);
  } else {
    const size_t lds = (size_t)(4 * 16 * WP + 4 * ((4 * (PT - 1) + KPAD / 4) * 4 + 16)) * 4;
    dim3 grid(persistent_blocks((long)p.nseq * p.tiles_per_seq, c->groups / 4), c->groups / 4);
    if (set_lds(&grouped_fwd<float>, lds)) return EVT_ELAUNCH;
    hipLaunchKernelGGL(grouped_fwd<float>, grid, dim3(256), lds, st, p);
  }
  return evt_check_launch();
}

// backward-data with an optional addend: dx = T(float(T(conv)) + float(dx_add))
extern "C" int evt_grouped_bwd_data_add(const evt_conv1d_params* c, const void* dy, const void* y, const void* w_reg,
                                        const void* dx_add, void* dx, void* stream) {
  GP p{};
  p.x = dy; p.xact = c->out_act != EVT_ACT_NONE ? y : nullptr; p.w = w_reg; p.y = dx; p.add = dx_add;
  p.nseq = c->nseq; p.lin = c->lin; p.lout = evt_conv1d_lout(c); p.cin = c->cin; p.cout = c->cout; p.k = c->k;
  p.pad = c->pad; p.groups = c->groups; p.in_slope = c->in_slope; p.out_act = c->out_act; p.out_slope = c->out_slope;
  p.cog = c->cout / c->groups;
  const int nq = (c->lin - 1 + c->pad) / 4 + 1;   // q' in [0, nq)
  p.tiles_per_seq = cdiv(nq, PT);
  hipStream_t st = (hipStream_t)stream;
  if (c->dtype == EVT_DT_HALF) {
    const int gb = groups_per_block(c->groups);
    p.lgp_x = ilog2(gb / 2); p.lgp_dy = ilog2(gb * p.cog / 8);
    p.nsplit = nq;
    const size_t lds = (size_t)gb * D_GARR * 2;
    dim3 grid(blocks16((long)p.nseq * p.tiles_per_seq, gb, c->groups / gb), c->groups / gb);
    if (set_lds(&grouped_bwd_data16, lds)) return EVT_ELAUNCH;
    hipLaunchKernelGGL(grouped_bwd_data16, grid, dim3(64 * gb), lds, st, p);
  } else {
    const size_t lds = (size_t)(4 * 16 * WP + 4 * ((PT + KPAD / 16 - 1) * 16 + 16)) * 4;
    dim3 grid(persistent_blocks((long)p.nseq * p.tiles_per_seq, c->groups / 4), c->groups / 4);
    if (set_lds(&grouped_bwd_data<float>, lds)) return EVT_ELAUNCH;
    hipLaunchKernelGGL(grouped_bwd_data<float>, grid, dim3(256), lds, st, p);
  }
  return evt_check_launch();
}

extern "C" int evt_grouped_bwd_data(const evt_conv1d_params* c, const void* dy, const void* y, const void* w_reg,
                                    void* dx, void* stream) {
  return evt_grouped_bwd_data_add(c, dy, y, w_reg, nullptr, dx, stream);
}

extern "C" int evt_grouped_bwd_weight(const evt_conv1d_params* c, const void* x, const void* dy, const void* y, float* dw,
                                      void* stream) {
  GP p{};
  p.x = x; p.dy = dy; p.xact = c->out_act != EVT_ACT_NONE ? y : nullptr; p.dw = dw;
  p.nseq = c->nseq; p.lin = c->lin; p.lout = evt_conv1d_lout(c); p.cin = c->cin; p.cout = c->cout; p.k = c->k;
  p.pad = c->pad; p.groups = c->groups; p.in_slope = c->in_slope; p.out_act = c->out_act; p.out_slope = c->out_slope;
  p.cog = c->cout / c->groups;
  p.tiles_per_seq = cdiv(p.lout, PT);
  const long total = (long)p.nseq * p.tiles_per_seq;
  const int sets = c->groups / 4;
  hipStream_t st = (hipStream_t)stream;
  if (c->dtype == EVT_DT_HALF) {
    // two blocks per CU over all group sets, at most one per CU for one set: every block adds its slice of dW with fp32
    // atomics, and `split` adders of one address serialise at the memory side -- with 4 groups (one set) 2 * CUs adders
    // cost more than the shorter chain of tiles saves.  At the benchmark's sizes a block walks 10 / 5 / 5 / 8 tiles,
    // prefetching each.
    long split = cdiv(2 * chip_cus(), sets);
    if (split > chip_cus()) split = chip_cus();
    if (split > total) split = total;
    if (split < 1) split = 1;
    p.nsplit = (int)split;
    p.lgp_x = 1; p.lgp_dy = ilog2(4 * p.cog / 8);
    const size_t lds_tr = (size_t)(4 * W_DARR + 4 * W_GARR) * 2;
    dim3 grid(p.nsplit, sets);
    if (set_lds(&grouped_bwd_weight_tr, lds_tr)) return EVT_ELAUNCH;
    hipLaunchKernelGGL(grouped_bwd_weight_tr, grid, dim3(256), lds_tr, st, p);
  } else {
    long split = 4 * chip_cus() / sets;
    if (split > chip_cus()) split = chip_cus();
    if (split < 16) split = 16;
    if (split > total) split = total;
    if (split < 1) split = 1;
    p.nsplit = (int)split;
    const size_t lds = (size_t)4 * (PT * 16 + (4 * (PT - 1) + 44) * 4 + 32) * 4;
    dim3 grid(p.nsplit, sets);
    if (set_lds(&grouped_bwd_weight<float>, lds)) return EVT_ELAUNCH;
    hipLaunchKernelGGL(grouped_bwd_weight<float>, grid, dim3(256), lds, st, p);
  }
  return evt_check_launch();
}

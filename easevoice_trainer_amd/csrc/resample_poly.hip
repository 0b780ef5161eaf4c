// The finishing launch of a ragged s2 decode: every row of the vocoder's output resampled to the requested rate by a
// polyphase windowed-sinc filter, converted to the requested sample format and packed, with a silence gap behind each
// row, into one buffer.  gfx950 only.
//
// Reference call site (file:line in the reference project):
//   int16 conversion, silence interval   src/easevoice/inference/tts.py:878-908 (audio_postprocess)
//
// The operator (include/evt.h has the definition): with c = m * down, q = c div up, p = c mod up and R = ceil(Z * max(up,
// down) / up), output m of a row of n live samples is
//     y[m] = sum_{j = 0}^{J - 1} T[p][j] * x[q - R + j]            x = 0 outside [0, n),  T[p][j] = g[p + (R - j) * up]
// T is built by the host in float64 and rounded once to fp32; its rows are padded with zeros to J, a multiple of 4.
//
// SUMMATION ORDER (fixed, a function of (m, up, down) only).  Four fp32 accumulators a0 .. a3 start at 0; for j = 0, 4,
// 8, ... in ascending order  a_e = fma(T[p][j + e], x[q - R + j + e], a_e)  for e = 0 .. 3; the result is
// (a0 + a1) + (a2 + a3).  Neither the number of rows, nor the row's place in the batch, nor the tile an output falls into
// enters: tiles start at the row's output 0, a tile only decides which block computes an output and where in LDS the
// samples lie.  The two forms of the kernel below (input span staged in LDS / read from global memory) run the same loop;
// which form runs is decided by (up, down) alone.
#include "evt_common.h"
#include "../../include/evt.h"

namespace {

constexpr int kTile = EVT_RESAMPLE_TILE;   // outputs (gap included) of one row per block
constexpr int kThreads = 256;
constexpr int kZeros = EVT_RESAMPLE_ZEROS;
constexpr int kLdsFloats = 12288;          // staged form while the input span of a tile fits 48 KB

enum { kIdentity = 0, kStaged = 1, kDirect = 2 };

// q = trunc(min(max(v * 32768, -32768), 32767)), NaN -> 0: the reference's (audio * 32768).astype(np.int16) with
// saturation in place of numpy's wrap-around
__device__ __forceinline__ int16_t pcm16(float v) {
  const float s = fminf(fmaxf(v * 32768.f, -32768.f), 32767.f);
  return v != v ? (int16_t)0 : (int16_t)(int)s;
}

template <typename O> __device__ __forceinline__ O to_out(float v);
template <> __device__ __forceinline__ float to_out<float>(float v) { return v; }
template <> __device__ __forceinline__ int16_t to_out<int16_t>(float v) { return pcm16(v); }

// grid (tiles of the longest possible row, nseq), 256 threads.  Block (t, s) owns positions [t * kTile, (t + 1) * kTile)
// of row s's To_s + gap output positions: resampled samples below To_s, zeros behind.  Lane l takes positions l, l + 256,
// ...: consecutive lanes store consecutive elements of `out` (the rows' offsets are not aligned to anything, so the
// stores are one element per lane, 128 / 256 contiguous bytes per wave).
// kStaged: the input span of the tile, x[q(m0) - R .. q(m_last) - R + J), is widened to fp32 once into LDS, zeros outside
// [0, n); the loop reads it without tests.  x is loaded one element per lane, coalesced: a 16-byte load would straddle the
// row's end, which must not be read, and the loads are < 1 % of the kernel's work.
// kDirect (ratios whose span does not fit): the same loop with x read from global memory under the same [0, n) test.
// kIdentity (up == down == 1): y[m] = x[m].
template <typename T, typename O, int MODE>
__global__ __launch_bounds__(kThreads) void resample_pack_kernel(const T* __restrict__ x, const int32_t* __restrict__ lens,
                                                                 int mul, long L, int up, int down, int R,
                                                                 const float* __restrict__ table, int J, O* __restrict__ out,
                                                                 long out_elems, const int64_t* __restrict__ out_off, int gap) {
  extern __shared__ __align__(16) float xs[];
  const int s = blockIdx.y;
  const long n = min(max((long)lens[s] * mul, 0L), L);
  const long To = n * up / down;
  const long m0 = (long)blockIdx.x * kTile;
  if (m0 >= To + gap) return;                                   // block-uniform
  const long m_end = min(m0 + kTile, To + gap);                 // positions of this block
  const long live_end = min(m_end, To);                         // ... of which resampled samples
  const long off = out_off[s];
  const T* xr = x + (long)s * L;
  long base = 0;
  if (MODE == kStaged && live_end > m0) {
    base = m0 * down / up - R;
    const int span = (int)((live_end - 1) * down / up - R + J - base);
    for (int i = threadIdx.x; i < span; i += kThreads) {
      const long src = base + i;
      xs[i] = (src >= 0 && src < n) ? to_f<T>(xr[src]) : 0.f;
    }
  }
  if (MODE == kStaged) __syncthreads();
  for (long m = m0 + threadIdx.x; m < m_end; m += kThreads) {
    float v = 0.f;
    if (m < To) {
      if (MODE == kIdentity) {
        v = to_f<T>(xr[m]);
      } else {
        const long c = m * down;
        const long q = c / up;
        const int p = (int)(c - q * up);
        const long i0 = q - R;
        const float4* t4 = reinterpret_cast<const float4*>(table + (long)p * J);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        if (MODE == kStaged) {
          const float* xl = xs + (i0 - base);
          for (int j = 0; j < J; j += 4) {
            const float4 t = t4[j >> 2];
            a0 = fmaf(t.x, xl[j], a0);
            a1 = fmaf(t.y, xl[j + 1], a1);
            a2 = fmaf(t.z, xl[j + 2], a2);
            a3 = fmaf(t.w, xl[j + 3], a3);
          }
        } else {
          // only the j whose sample lies in [0, n): the others add fma(t, 0, a) = a
          const int jlo = (int)max(0L, -i0) & ~3;
          const int jhi = (int)min((long)J, n - i0);
          for (int j = jlo; j < jhi; j += 4) {
            const float4 t = t4[j >> 2];
            const long i = i0 + j;
            a0 = fmaf(t.x, (i >= 0 && i < n) ? to_f<T>(xr[i]) : 0.f, a0);
            a1 = fmaf(t.y, (i + 1 >= 0 && i + 1 < n) ? to_f<T>(xr[i + 1]) : 0.f, a1);
            a2 = fmaf(t.z, (i + 2 >= 0 && i + 2 < n) ? to_f<T>(xr[i + 2]) : 0.f, a2);
            a3 = fmaf(t.w, (i + 3 >= 0 && i + 3 < n) ? to_f<T>(xr[i + 3]) : 0.f, a3);
          }
        }
        v = (a0 + a1) + (a2 + a3);
      }
    }
    const long at = off + m;
    if (at >= 0 && at < out_elems) out[at] = to_out<O>(v);      // never outside the buffer, whatever out_off holds
  }
}

template <typename T, typename O>
void launch_mode(int mode, dim3 grid, size_t lds, hipStream_t st, const void* x, const int32_t* lens, int mul, long L, int up,
                 int down, int R, const float* table, int J, void* out, long out_elems, const int64_t* out_off, int gap) {
  if (mode == kIdentity)
    hipLaunchKernelGGL((resample_pack_kernel<T, O, kIdentity>), grid, dim3(kThreads), 0, st, (const T*)x, lens, mul, L, up,
                       down, R, table, J, (O*)out, out_elems, out_off, gap);
  else if (mode == kStaged)
    hipLaunchKernelGGL((resample_pack_kernel<T, O, kStaged>), grid, dim3(kThreads), lds, st, (const T*)x, lens, mul, L, up,
                       down, R, table, J, (O*)out, out_elems, out_off, gap);
  else
    hipLaunchKernelGGL((resample_pack_kernel<T, O, kDirect>), grid, dim3(kThreads), 0, st, (const T*)x, lens, mul, L, up,
                       down, R, table, J, (O*)out, out_elems, out_off, gap);
}

}  // namespace

extern "C" {

int evt_resample_pack_rows(int32_t dtype, const void* x, const int32_t* lens, int32_t mul, int32_t nseq, int32_t L,
                           int32_t up, int32_t down, const float* table, int32_t J, int32_t out_format, void* out,
                           int64_t out_elems, const int64_t* out_off, int32_t gap, void* stream) {
  if (!x || !lens || !out || !out_off || nseq <= 0 || nseq > 65535 || L <= 0 || mul <= 0 || up <= 0 || down <= 0 ||
      out_elems <= 0 || gap < 0)
    return EVT_EINVAL;
  if (dtype != EVT_DT_HALF && dtype != EVT_DT_F32) return EVT_EINVAL;
  if (out_format != EVT_PCM_F32 && out_format != EVT_PCM_S16) return EVT_EINVAL;
  const int in_size = dtype == EVT_DT_F32 ? 4 : 2, out_size = out_format == EVT_PCM_F32 ? 4 : 2;
  if (((uintptr_t)x & (in_size - 1)) || ((uintptr_t)out & (out_size - 1)) || ((uintptr_t)lens & 3) || ((uintptr_t)out_off & 7))
    return EVT_EINVAL;
  int mode = kIdentity, R = 0;
  size_t lds = 0;
  if (up != 1 || down != 1) {
    // R = ceil(Z * max(up, down) / up); a table row holds the 2 R + 1 taps of a phase, padded with zeros to J % 4 == 0
    const long H = (long)kZeros * (up > down ? up : down);
    const long r = (H + up - 1) / up;
    if (!table || ((uintptr_t)table & 15) || J % 4 || J < 2 * r + 1 || J > 2 * r + 4) return EVT_EINVAL;
    R = (int)r;
    const long span = (long)(kTile - 1) * down / up + 1 + J;   // most input samples one tile reads
    mode = span <= kLdsFloats ? kStaged : kDirect;
    lds = mode == kStaged ? (size_t)span * sizeof(float) : 0;
  }
  const long max_to = (long)L * up / down;                       // the longest row a launch can hold
  const long tiles = (max_to + gap + kTile - 1) / kTile;
  if (tiles <= 0) return EVT_EINVAL;                             // no row can hold a sample and gap == 0: nothing to write
  if (tiles > 0x7fffffffL) return EVT_EINVAL;
  const dim3 grid((unsigned)tiles, (unsigned)nseq);
  hipStream_t st = (hipStream_t)stream;
#define EVT_RP_LAUNCH(T, O) \
  launch_mode<T, O>(mode, grid, lds, st, x, lens, mul, (long)L, up, down, R, table, J, out, (long)out_elems, out_off, gap)
  if (dtype == EVT_DT_HALF) {
    if (out_format == EVT_PCM_S16) EVT_RP_LAUNCH(h16_t, int16_t);
    else EVT_RP_LAUNCH(h16_t, float);
  } else {
    if (out_format == EVT_PCM_S16) EVT_RP_LAUNCH(float, int16_t);
    else EVT_RP_LAUNCH(float, float);
  }
#undef EVT_RP_LAUNCH
  return evt_check_launch();
}

}  // extern "C"

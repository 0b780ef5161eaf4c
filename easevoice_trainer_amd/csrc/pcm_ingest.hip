// The first launch of the audio pipeline: the sample bytes of WAV recordings -- any of six encodings, 1 .. 8 channels,
// any rate -- decoded, mixed down to mono and resampled to the pipeline's rate into the packed fp32 buffer the slicer and
// the later stages read.  gfx950 only.
//
// Reference call sites (file:line in the reference project):
//   load_audio: ffmpeg, ac=1, ar=sr                       src/utils/audio/__init__.py:13-32
//   librosa.load(path, sr=16000) of the prompt clip       src/easevoice/inference/tts.py:411-437 (_set_prompt_semantic)
//
// The operator (include/evt.h has the definition): frame i of a recording is decoded sample by sample to fp32 (exact, or
// one round-to-nearest-even), the channels are added in channel order and divided by their number,
//     m[i] = fdiv(((v_0 + v_1) + ...) + v_{C-1}, (float)C)
// and m[0 .. frames) goes through the resampler of csrc/resample_poly.hip unchanged: the same table, the same four
// accumulators, the same (a0 + a1) + (a2 + a3).  The kernel below has that file's shape -- a block owns EVT_RESAMPLE_TILE
// outputs of one recording counted from its output 0; the staged form decodes the tile's input span once into LDS, the
// direct form decodes from global memory per tap; (up, down) alone decide which runs -- with the decode in place of its
// load.  Format and channel count are read per recording and are block-uniform: the switch on them does not diverge.
//
// Loads.  Samples are read one at a time with a load of the sample's own size where the recording's first byte is aligned
// to it (the host's staging aligns every recording to 16 bytes) and byte by byte otherwise and for the 3-byte format.  A
// load never covers a byte of another sample, so none straddles the recording's end.  Consecutive lanes take consecutive
// frames: a wave's loads fall into the same few cache lines.  The launch is bound by the upload in front of it
// (profiles/ingest_batch.json), not by these loads.
#include "evt_common.h"
#include "../../include/evt.h"

namespace {

constexpr int kTile = EVT_RESAMPLE_TILE;
constexpr int kThreads = 256;
constexpr int kZeros = EVT_RESAMPLE_ZEROS;
constexpr int kLdsFloats = 12288;          // staged form while the input span of a tile fits 48 KB (resample_poly.hip's rule)

enum { kIdentity = 0, kStaged = 1, kDirect = 2 };

__device__ __forceinline__ int width_of(int fmt) {
  return fmt == EVT_PCM_IN_U8 ? 1 : fmt == EVT_PCM_IN_S16 ? 2 : fmt == EVT_PCM_IN_S24 ? 3 : fmt == EVT_PCM_IN_F64 ? 8 : 4;
}

// `w` little-endian bytes at p as an unsigned integer; ALIGNED: p is a multiple of w (w a power of two), one load
template <bool ALIGNED> __device__ __forceinline__ uint64_t load_le(const uint8_t* p, int w) {
  if (ALIGNED) {
    if (w == 2) return *reinterpret_cast<const uint16_t*>(p);
    if (w == 4) return *reinterpret_cast<const uint32_t*>(p);
    if (w == 8) return *reinterpret_cast<const uint64_t*>(p);
  }
  uint64_t v = 0;
  for (int b = 0; b < w; ++b) v |= (uint64_t)p[b] << (8 * b);
  return v;
}

// one sample -> fp32: exact, or one round-to-nearest-even (s32, f64); NaN and infinities pass, nothing is clamped
template <bool ALIGNED> __device__ __forceinline__ float decode(const uint8_t* p, int fmt) {
  switch (fmt) {
    case EVT_PCM_IN_U8: return (float)((int)p[0] - 128) * 0x1p-7f;
    case EVT_PCM_IN_S16: return (float)(int16_t)load_le<ALIGNED>(p, 2) * 0x1p-15f;
    case EVT_PCM_IN_S24: return (float)((int32_t)((uint32_t)load_le<false>(p, 3) << 8) >> 8) * 0x1p-23f;
    case EVT_PCM_IN_S32: return (float)(int32_t)load_le<ALIGNED>(p, 4) * 0x1p-31f;
    case EVT_PCM_IN_F32: return __uint_as_float((uint32_t)load_le<ALIGNED>(p, 4));
    default: return (float)__longlong_as_double((long long)load_le<ALIGNED>(p, 8));
  }
}

// frame i of a recording whose first byte is `rec`: the channels added in channel order, each sum rounded to fp32, one
// correctly rounded division (a mono frame is its sample: x / 1 = x, and the bits of a NaN stay as they are)
template <bool ALIGNED> __device__ __forceinline__ float mono(const uint8_t* rec, long i, int fmt, int ch, int w) {
  const uint8_t* p = rec + i * (long)(ch * w);
  float acc = decode<ALIGNED>(p, fmt);
  if (ch == 1) return acc;
  for (int c = 1; c < ch; ++c) acc = __fadd_rn(acc, decode<ALIGNED>(p + c * w, fmt));
  return __fdiv_rn(acc, (float)ch);
}

// grid (tiles of the longest possible recording, nrec), 256 threads.  Block (t, r) owns outputs [t * kTile, (t + 1) *
// kTile) of recording r; lane l takes l, l + 256, ...: consecutive lanes store consecutive elements of `out`.
// kStaged: m[q(m0) - R .. q(m_last) - R + J) into LDS, zeros outside [0, n); the tap loop reads it without tests.
// kDirect (ratios whose span does not fit): the same loop, m[i] decoded from global memory under the [0, n) test.
// kIdentity (up == down == 1): y[i] = m[i].
template <int MODE, bool ALIGNED>
__device__ __forceinline__ void ingest_tile(const uint8_t* __restrict__ rec, long n, int fmt, int ch, int w, int up, int down,
                                            int R, const float* __restrict__ table, int J, float* __restrict__ out,
                                            long out_elems, long off, float* xs) {
  const long To = n * up / down;
  const long m0 = (long)blockIdx.x * kTile;
  if (m0 >= To) return;                                         // block-uniform
  const long m_end = min(m0 + kTile, To);
  long base = 0;
  if (MODE == kStaged) {
    base = m0 * down / up - R;
    const int span = (int)((m_end - 1) * down / up - R + J - base);
    for (int i = threadIdx.x; i < span; i += kThreads) {
      const long src = base + i;
      xs[i] = (src >= 0 && src < n) ? mono<ALIGNED>(rec, src, fmt, ch, w) : 0.f;
    }
    __syncthreads();
  }
  for (long m = m0 + threadIdx.x; m < m_end; m += kThreads) {
    float v;
    if (MODE == kIdentity) {
      v = mono<ALIGNED>(rec, m, fmt, ch, w);
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
          a0 = fmaf(t.x, (i >= 0 && i < n) ? mono<ALIGNED>(rec, i, fmt, ch, w) : 0.f, a0);
          a1 = fmaf(t.y, (i + 1 >= 0 && i + 1 < n) ? mono<ALIGNED>(rec, i + 1, fmt, ch, w) : 0.f, a1);
          a2 = fmaf(t.z, (i + 2 >= 0 && i + 2 < n) ? mono<ALIGNED>(rec, i + 2, fmt, ch, w) : 0.f, a2);
          a3 = fmaf(t.w, (i + 3 >= 0 && i + 3 < n) ? mono<ALIGNED>(rec, i + 3, fmt, ch, w) : 0.f, a3);
        }
      }
      v = (a0 + a1) + (a2 + a3);
    }
    const long at = off + m;
    if (at >= 0 && at < out_elems) out[at] = v;                 // never outside the buffer, whatever out_off holds
  }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void pcm_ingest_kernel(const uint8_t* __restrict__ raw, long raw_len,
                                                              const int64_t* __restrict__ byte_off,
                                                              const int64_t* __restrict__ frames,
                                                              const int32_t* __restrict__ fmts,
                                                              const int32_t* __restrict__ channels, long max_frames, int up,
                                                              int down, int R, const float* __restrict__ table, int J,
                                                              float* __restrict__ out, long out_elems,
                                                              const int64_t* __restrict__ out_off) {
  extern __shared__ __align__(16) float xs[];
  const int r = blockIdx.y;
  const int fmt = fmts[r], ch = channels[r];
  if (fmt < EVT_PCM_IN_U8 || fmt > EVT_PCM_IN_F64 || ch < 1 || ch > EVT_PCM_IN_MAX_CHANNELS) return;   // block-uniform
  const int w = width_of(fmt);
  const long n = min(max((long)frames[r], 0L), max_frames);
  const long boff = byte_off[r];
  // the recording's bytes lie inside the buffer, or nothing of it is read (a division: no product can overflow)
  if (boff < 0 || boff > raw_len || n > (raw_len - boff) / (ch * w)) return;
  const uint8_t* rec = raw + boff;
  const long off = out_off[r];
  if (((uintptr_t)rec & (uintptr_t)(w - 1)) == 0 && w != 3)
    ingest_tile<MODE, true>(rec, n, fmt, ch, w, up, down, R, table, J, out, out_elems, off, xs);
  else
    ingest_tile<MODE, false>(rec, n, fmt, ch, w, up, down, R, table, J, out, out_elems, off, xs);
}

}  // namespace

extern "C" {

int evt_pcm_ingest_rows(const uint8_t* raw, int64_t raw_len, const int64_t* byte_off, const int64_t* frames,
                        const int32_t* fmt, const int32_t* channels, int32_t nrec, int64_t max_frames, int32_t up,
                        int32_t down, const float* table, int32_t J, float* out, int64_t out_elems, const int64_t* out_off,
                        void* stream) {
  if (!raw || !byte_off || !frames || !fmt || !channels || !out || !out_off || raw_len <= 0 || nrec <= 0 || nrec > 65535 ||
      max_frames <= 0 || max_frames > 0x7fffffffL || up <= 0 || down <= 0 || out_elems <= 0)
    return EVT_EINVAL;
  if (((uintptr_t)out & 3) || ((uintptr_t)fmt & 3) || ((uintptr_t)channels & 3) || ((uintptr_t)byte_off & 7) ||
      ((uintptr_t)frames & 7) || ((uintptr_t)out_off & 7))
    return EVT_EINVAL;
  int mode = kIdentity, R = 0;
  size_t lds = 0;
  if (up != 1 || down != 1) {
    // R = ceil(Z * max(up, down) / up); a table row holds the 2 R + 1 taps of a phase, padded with zeros to J % 4 == 0
    const long H = (long)kZeros * (up > down ? up : down);
    const long r = (H + up - 1) / up;
    if (!table || ((uintptr_t)table & 15) || J % 4 || J < 2 * r + 1 || J > 2 * r + 4) return EVT_EINVAL;
    R = (int)r;
    const long span = (long)(kTile - 1) * down / up + 1 + J;   // most input frames one tile reads
    mode = span <= kLdsFloats ? kStaged : kDirect;
    lds = mode == kStaged ? (size_t)span * sizeof(float) : 0;
  }
  const long max_to = (long)max_frames * up / down;              // the longest recording a launch can hold
  const long tiles = (max_to + kTile - 1) / kTile;
  if (tiles <= 0) return EVT_OK;                                 // no recording can give a sample: nothing to write
  if (tiles > 0x7fffffffL) return EVT_EINVAL;
  const dim3 grid((unsigned)tiles, (unsigned)nrec);
  hipStream_t st = (hipStream_t)stream;
#define EVT_PI_LAUNCH(MODE, LDS)                                                                                        \
  hipLaunchKernelGGL((pcm_ingest_kernel<MODE>), grid, dim3(kThreads), LDS, st, raw, (long)raw_len, byte_off, frames, fmt, \
                     channels, (long)max_frames, up, down, R, table, J, out, (long)out_elems, out_off)
  if (mode == kIdentity) EVT_PI_LAUNCH(kIdentity, 0);
  else if (mode == kStaged) EVT_PI_LAUNCH(kStaged, lds);
  else EVT_PI_LAUNCH(kDirect, 0);
#undef EVT_PI_LAUNCH
  return evt_check_launch();
}

}  // extern "C"

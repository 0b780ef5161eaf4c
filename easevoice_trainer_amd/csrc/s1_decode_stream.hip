// s1 decoding with PER-ROW counters: the step of a continuously batched session (auto_reg/t2s_infer.py StreamSession), in
// which a finished row's slot is refilled with the next waiting text while the other rows keep decoding, for gfx950.
//
// The sessions of s1_decode.hip keep one set of counters ctr[POS|IDX|YCOUNT|YLEN] for all rows, so every row has the
// same prompt length and the same step index, and the counters may only move in a launch of their own after every row's
// workgroup has read them.  Here every row b owns rstate[b][8] (EVT_ROW_*): cache position, step index, token count,
// prompt length, step limit, status and the column of an injected noise table.  A row is touched only by its own
// workgroups, so
//   dec_attn_rows          is dec_attn with pos = rstate[b][POS]; a row that is not running returns at once;
//   dec_sample_embed_rows  samples, appends, tests EOS / the step limit, embeds the next input and moves the row's
//                          counters in ONE launch for all rows (three launches in a session with shared counters);
//   dec_sample_embed_rows_p  is the same launch with top_k / top_p / temperature / repetition_penalty of row b read from
//                          a device table row_sample[b], so requests of one session sample with their own values and
//                          the captured step graph does not depend on them;
//   dec_sample_embed_rows_lp is that launch again, which also writes the step's two log-probabilities of the drawn token
//                          to row_logp[b][YCOUNT]: log_softmax of the raw logits (the model's) and the log of the
//                          probability it was drawn from after penalty, nucleus, top-k and temperature (the sampler's).
//   dec_sample_embed_rows_f is the _p / _lp launch (without / with row_logp) in which a row may have FORCED steps: while
//                          IDX < rstate[b][NFORCE] the row's token is the one the host wrote at y[b][YCOUNT], not the
//                          draw -- scoring a given take, resuming a preempted row, continuing a given prefix.
// A row that stops (EOS, or its limit) is marked in the same launch and is skipped from then on: however late the host
// reads the status, a stopped row never advances its position or writes past its buffers.
// The counters are written with ordinary stores by thread 0 of the row's workgroup after a barrier.
#include "s1_decode_common.h"

namespace {

template <typename T, int D>
__global__ __launch_bounds__(256) void dec_attn_rows(const float* __restrict__ qkv, T* kc, T* vc,
                                                     const int* __restrict__ rstate, float* __restrict__ out, int H,
                                                     int Lmax, const int* __restrict__ x_lens, int x_len) {
  extern __shared__ float sc[];   // [Lmax] scores -> probabilities
  __shared__ float qs[D], kn[D], vn[D], red[4], part[AttnShape<T, D>::G][D + 1];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / H, h = blockIdx.x % H, E = H * D;
  const int* rs = rstate + b * EVT_ROW_WORDS;
  if (rs[EVT_ROW_STATUS] != EVT_ROW_RUNNING) return;   // idle / stopped: no cache write, out untouched
  const int pos = rs[EVT_ROW_POS];
  if (pos < 0 || pos >= Lmax) return;   // cache full: the host bounds the number of steps, this only guards memory
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

struct RowEmbed { const float* emb; const float* pe; const float* alpha; float* x; float x_scale; int E, npos, dpos; };

// The end of a step for row b = blockIdx.x, shared by the two kernels below.  `p` is this workgroup's own copy of the
// sampling parameters: the session-wide one, or that copy with the row's four values written over it.  kLp is a
// compile-time switch, so the two kernels without log-probabilities compile the body they always had; with it, the raw
// logits get a block_max / block_sum of their own before the sampler touches anything, and thread 0 adds two stores.
// kForce is a second such switch (dec_sample_embed_rows_f): in a step with IDX < rstate[b][NFORCE] the token is the
// one found at yb[ycount] and the arg-max EOS rule is off; without it the body is the one compiled before.
template <bool kLp = false, bool kForce = false>
__device__ __forceinline__ void sample_embed_row(const evt_sample_params& p, const float* __restrict__ logits, long* y,
                                                 int* rs, const float* __restrict__ noise, int* stop_idx,
                                                 float* probs_out, const int* __restrict__ row_seed, const RowEmbed& ea,
                                                 float* row_logp = nullptr) {
  const int tid = threadIdx.x, b = blockIdx.x, V = p.V;
  const int idx = rs[EVT_ROW_IDX], ycount = rs[EVT_ROW_YCOUNT], ylen = rs[EVT_ROW_YLEN], limit = rs[EVT_ROW_LIMIT];
  int col = rs[EVT_ROW_NOISE];
  if (col < 0 || col >= p.noise_rows) col = 0;
  long* yb = y + (long)b * p.ymax;
  // A forced step takes its token from the row's own y buffer.  rs and yb are addressed by blockIdx.x alone and idx,
  // ycount are the same words on every thread, so `given` is uniform over the workgroup; it decides no barrier anyway
  // (it selects which column's log-probability is reported, and the token after the draw).  The value becomes an index
  // of the embedding table and of the logits: anything outside [0, V) is replaced by the marker the all-NaN arg-max
  // leaves (0x7fffffff), which is stored for the host to see, embeds row 0 and reports NaN log-probabilities.
  int given = -1;
  if constexpr (kForce) {
    if (idx < rs[EVT_ROW_NFORCE] && ycount >= 0 && ycount < p.ymax) {
      const long t = yb[ycount];
      given = t >= 0 && t < V ? (int)t : 0x7fffffff;
    }
  }
  int amax;
  float rmax = -INFINITY, rlsum = 0.f;   // max and log(sum exp(. - max)) of the raw logits over this step's Ve columns
  float* lpsh = nullptr;                 // LDS word for the sampler's log-probability; only the kLp kernel has it
  if constexpr (kLp) {
    __shared__ float lp_lds[17];
    lpsh = lp_lds + 16;
    const float* lg = logits + (long)b * V;
    const int Ve = idx < p.no_eos_steps ? V - 1 : V;
    for (int v = tid; v < Ve; v += 1024) rmax = fmaxf(rmax, lg[v]);
    rmax = block_max(rmax, lp_lds, 16);
    for (int v = tid; v < Ve; v += 1024) rlsum += expf(lg[v] - rmax);
    rlsum = logf(block_sum(rlsum, lp_lds, 16));
    if (tid == 0) lpsh[0] = NAN;   // stays when no thread owns the token (all-NaN probabilities)
  }
  int tok = sample_row<kLp, kForce>(p, logits + (long)b * V, yb, idx, ycount, (unsigned)row_seed[2 * b],
                                    (unsigned)row_seed[2 * b + 1],
                                    noise ? noise + ((long)idx * p.noise_rows + col) * V : nullptr,
                                    probs_out ? probs_out + (long)b * V : nullptr, &amax, lpsh, given);
  if constexpr (kForce) {
    if (given >= 0) tok = given;   // the draw is dropped; everything below sees the given token
  }
  // x_next = emb[token] * x_scale + alpha * pe[y_len + idx]  (t2s_model.py:860-861)
  int ppos = ylen + idx;
  if (ppos >= ea.npos) ppos = ea.npos - 1;
  const float al = ea.alpha[0];
  // the rounding is spelled out (one product rounded, then one fused multiply-add) instead of left to the compiler's
  // contraction, which picks different forms for different loop shapes: this is what dec_embed computes at E = 512
  // sample_row's arg-max leaves its start value 0x7fffffff when every probability is NaN (NaN logits, or a NaN among
  // the sampling parameters): the token is stored as it is for the host to see, the embedding row is kept in range
  const int trow = (unsigned)tok < (unsigned)V ? tok : 0;
  for (int c = tid; c < ea.E; c += 1024)
    ea.x[(long)b * ea.E + c] =
        __fmaf_rn(ea.emb[(long)trow * ea.E + c], ea.x_scale, __fmul_rn(al, ea.pe[(long)ppos * ea.E + c]));
  __syncthreads();       // every read of the row's state above is done; only this workgroup touches it
  if (tid == 0) {
    if (ycount < p.ymax) yb[ycount] = tok;
    if constexpr (kLp) {
      if (ycount < p.ymax) {
        const bool ok = (unsigned)tok < (unsigned)V;
        float* o = row_logp + ((long)b * p.ymax + ycount) * 2;
        o[0] = ok ? logits[(long)b * V + tok] - rmax - rlsum : NAN;
        o[1] = ok ? lpsh[0] : NAN;
        if constexpr (kForce) {   // a given token outside the step's Ve columns (EOS at a step without it): no mass
          if (given >= 0 && ok && tok >= (idx < p.no_eos_steps ? V - 1 : V)) o[0] = -INFINITY;
        }
      }
    }
    bool by_amax = amax == p.eos;
    if constexpr (kForce) {
      if (given >= 0) by_amax = false;   // the given sequence decides where it ends, not the model's arg-max
    }
    if (by_amax || tok == p.eos) {
      stop_idx[b] = idx;
      rs[EVT_ROW_STATUS] = EVT_ROW_STOP_EOS;
    } else if (idx + 1 >= limit || ycount + 1 >= p.ymax) {
      stop_idx[b] = idx;
      rs[EVT_ROW_STATUS] = EVT_ROW_STOP_LIMIT;
    } else {
      rs[EVT_ROW_POS] += ea.dpos;
      rs[EVT_ROW_IDX] = idx + 1;
      rs[EVT_ROW_YCOUNT] = ycount + 1;
    }
  }
}

__global__ __launch_bounds__(1024) void dec_sample_embed_rows(evt_sample_params p, const float* __restrict__ logits,
                                                              long* y, int* rstate, const float* __restrict__ noise,
                                                              int* stop_idx, float* probs_out,
                                                              const int* __restrict__ row_seed,
                                                              const int* __restrict__ row_mask, RowEmbed ea) {
  const int b = blockIdx.x;
  if (row_mask && !row_mask[b]) return;
  int* rs = rstate + b * EVT_ROW_WORDS;
  if (rs[EVT_ROW_STATUS] != EVT_ROW_RUNNING) return;
  sample_embed_row(p, logits, y, rs, noise, stop_idx, probs_out, row_seed, ea);
}

// dec_sample_embed_rows with top_k / top_p / temperature / repetition_penalty of row b taken from row_sample[b]
__global__ __launch_bounds__(1024) void dec_sample_embed_rows_p(evt_sample_params p,
                                                                const evt_row_sample* __restrict__ row_sample,
                                                                const float* __restrict__ logits, long* y, int* rstate,
                                                                const float* __restrict__ noise, int* stop_idx,
                                                                float* probs_out, const int* __restrict__ row_seed,
                                                                const int* __restrict__ row_mask, RowEmbed ea) {
  const int b = blockIdx.x;
  if (row_mask && !row_mask[b]) return;
  int* rs = rstate + b * EVT_ROW_WORDS;
  if (rs[EVT_ROW_STATUS] != EVT_ROW_RUNNING) return;
  // One 16-byte entry per row, addressed by blockIdx.x alone: every thread of the workgroup loads the same four values,
  // so the branches of sample_row on them (repetition_penalty != 1, top_p < 1, top_k > 0) are taken by all 1024 threads
  // or by none, and the barriers inside `if (p.top_p < 1.0f)` stay non-divergent, as with the by-value parameters.
  // No table value can move an address out of bounds.  top_k only selects si[kk - 1] after the clamp 1 <= kk <= Ve
  // (top_k <= 0 skips the pivot), and si[] holds the sort's own indices 0..kSortN-1 into cur[kSortN].  top_p,
  // temperature and repetition_penalty feed comparisons, multiplications and divisions of values, never an index.  The
  // one index derived from those values is the token: with NaN probabilities the arg-max returns 0x7fffffff, which
  // sample_embed_row keeps away from the embedding table and which only lands in the row's own y slot.  The host still
  // refuses non-finite values and repetition_penalty <= 0 before they reach the table.
  const evt_row_sample r = row_sample[b];
  p.top_k = r.top_k;
  p.top_p = r.top_p;
  p.temperature = r.temperature;
  p.repetition_penalty = r.repetition_penalty;
  sample_embed_row(p, logits, y, rs, noise, stop_idx, probs_out, row_seed, ea);
}

// dec_sample_embed_rows_p that also records the two log-probabilities of the drawn token at row_logp[b][YCOUNT][0..1]
// (YCOUNT as read before the counters move: the index at which the token is appended to y).  Rows that return early
// write nothing.  y, rstate, stop_idx, x and probs_out are those of dec_sample_embed_rows_p bit for bit: the sampler
// runs the same instructions on the same values, the extra reductions only read the logits.
__global__ __launch_bounds__(1024) void dec_sample_embed_rows_lp(evt_sample_params p,
                                                                 const evt_row_sample* __restrict__ row_sample,
                                                                 const float* __restrict__ logits, long* y, int* rstate,
                                                                 const float* __restrict__ noise, int* stop_idx,
                                                                 float* probs_out, const int* __restrict__ row_seed,
                                                                 const int* __restrict__ row_mask, RowEmbed ea,
                                                                 float* row_logp) {
  const int b = blockIdx.x;
  if (row_mask && !row_mask[b]) return;
  int* rs = rstate + b * EVT_ROW_WORDS;
  if (rs[EVT_ROW_STATUS] != EVT_ROW_RUNNING) return;
  const evt_row_sample r = row_sample[b];   // uniform over the workgroup, see dec_sample_embed_rows_p
  p.top_k = r.top_k;
  p.top_p = r.top_p;
  p.temperature = r.temperature;
  p.repetition_penalty = r.repetition_penalty;
  sample_embed_row<true>(p, logits, y, rs, noise, stop_idx, probs_out, row_seed, ea, row_logp);
}

// dec_sample_embed_rows_p (kLp = false, row_logp unused) or dec_sample_embed_rows_lp (kLp = true) with forced steps:
// row b takes the token at y[b][YCOUNT] instead of its draw while IDX < rstate[b][EVT_ROW_NFORCE].  The step index
// keeps counting through forced steps and keys the noise as ever, so the first sampled step after k forced ones reads
// noise row k: a row resumed from a forced prefix draws what it would have drawn had it sampled that prefix itself.
// NFORCE is read through rs (blockIdx.x alone), so the workgroup-uniformity argument of dec_sample_embed_rows_p holds:
// no barrier of sample_row depends on it.  With NFORCE = 0 every value is that of the _p / _lp kernel bit for bit.
template <bool kLp>
__global__ __launch_bounds__(1024) void dec_sample_embed_rows_f(evt_sample_params p,
                                                                const evt_row_sample* __restrict__ row_sample,
                                                                const float* __restrict__ logits, long* y, int* rstate,
                                                                const float* __restrict__ noise, int* stop_idx,
                                                                float* probs_out, const int* __restrict__ row_seed,
                                                                const int* __restrict__ row_mask, RowEmbed ea,
                                                                float* row_logp) {
  const int b = blockIdx.x;
  if (row_mask && !row_mask[b]) return;
  int* rs = rstate + b * EVT_ROW_WORDS;
  if (rs[EVT_ROW_STATUS] != EVT_ROW_RUNNING) return;
  const evt_row_sample r = row_sample[b];   // uniform over the workgroup, see dec_sample_embed_rows_p
  p.top_k = r.top_k;
  p.top_p = r.top_p;
  p.temperature = r.temperature;
  p.repetition_penalty = r.repetition_penalty;
  sample_embed_row<kLp, true>(p, logits, y, rs, noise, stop_idx, probs_out, row_seed, ea, row_logp);
}

}  // namespace

// The host side of the four evt_dec_sample_embed_rows* entry points: the common validation, RowEmbed, the noise_rows
// clamp and the choice of the kernel.  What differs per entry point: only kRows takes the four sampling values by value
// and so refuses repetition_penalty <= 0 (the others read them from row_sample in device memory: the host that fills the
// table validates them, t2s_infer.py); kRowsLp needs row_logp; kRowsF accepts NULL for it (the _p body) -- its forced
// tokens live in y, device memory: the host that writes them validates them, the kernel clamps them.
enum RowsEntry { kRows, kRowsP, kRowsLp, kRowsF };

static int launch_sample_embed_rows(RowsEntry which, const evt_sample_params* p, const evt_row_sample* row_sample,
                                    const float* logits, int64_t* y, int32_t* rstate, const float* noise,
                                    int32_t* stop_idx, float* probs_out, const int32_t* row_seed, const int32_t* row_mask,
                                    const float* emb, const float* pe, const float* alpha, float x_scale, float* x,
                                    float* row_logp, int32_t B, int32_t E, int32_t npos, int32_t dpos, void* stream) {
  if (!p || !logits || !y || !rstate || !stop_idx || !row_seed || !emb || !pe || !alpha || !x || B <= 0 || E <= 0 ||
      npos <= 0 || dpos < 0)
    return EVT_EINVAL;
  if ((which != kRows && !row_sample) || (which == kRowsLp && !row_logp)) return EVT_EINVAL;
  if (p->V <= 1 || p->V > kSortN || p->ymax <= 0 || (which == kRows && p->repetition_penalty <= 0.f)) return EVT_EINVAL;
  RowEmbed ea{emb, pe, alpha, x, x_scale, E, npos, dpos};
  evt_sample_params sp = *p;
  if (sp.noise_rows < 1) sp.noise_rows = 1;
  const dim3 grid(B), block(1024);
  hipStream_t st = (hipStream_t)stream;
  if (which == kRows)
    hipLaunchKernelGGL(dec_sample_embed_rows, grid, block, 0, st, sp, logits, (long*)y, rstate, noise, stop_idx,
                       probs_out, row_seed, row_mask, ea);
  else if (which == kRowsP)
    hipLaunchKernelGGL(dec_sample_embed_rows_p, grid, block, 0, st, sp, row_sample, logits, (long*)y, rstate, noise,
                       stop_idx, probs_out, row_seed, row_mask, ea);
  else if (which == kRowsLp)
    hipLaunchKernelGGL(dec_sample_embed_rows_lp, grid, block, 0, st, sp, row_sample, logits, (long*)y, rstate, noise,
                       stop_idx, probs_out, row_seed, row_mask, ea, row_logp);
  else if (row_logp)
    hipLaunchKernelGGL(dec_sample_embed_rows_f<true>, grid, block, 0, st, sp, row_sample, logits, (long*)y, rstate, noise,
                       stop_idx, probs_out, row_seed, row_mask, ea, row_logp);
  else
    hipLaunchKernelGGL(dec_sample_embed_rows_f<false>, grid, block, 0, st, sp, row_sample, logits, (long*)y, rstate,
                       noise, stop_idx, probs_out, row_seed, row_mask, ea, row_logp);
  return evt_check_launch();
}

extern "C" {

int evt_dec_attn_rows(int32_t cdtype, const float* qkv, void* kcache, void* vcache, const int32_t* rstate, float* out,
                      int32_t B, int32_t H, int32_t D, int32_t Lmax, const int32_t* x_lens, int32_t x_len, void* stream) {
  if (!qkv || !kcache || !vcache || !rstate || !out || B <= 0 || H <= 0 || Lmax <= 0) return EVT_EINVAL;
  if (D != 32 || (size_t)Lmax * 4 > 60 * 1024) return EVT_ENOTSUP;
  const size_t shm = (size_t)Lmax * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (cdtype == EVT_DT_HALF)
    hipLaunchKernelGGL((dec_attn_rows<h16_t, 32>), dim3(B * H), dim3(256), shm, st, qkv, (h16_t*)kcache, (h16_t*)vcache,
                       (const int*)rstate, out, H, Lmax, (const int*)x_lens, x_len);
  else if (cdtype == EVT_DT_F32)
    hipLaunchKernelGGL((dec_attn_rows<float, 32>), dim3(B * H), dim3(256), shm, st, qkv, (float*)kcache, (float*)vcache,
                       (const int*)rstate, out, H, Lmax, (const int*)x_lens, x_len);
  else return EVT_EINVAL;
  return evt_check_launch();
}

int evt_dec_sample_embed_rows(const evt_sample_params* p, const float* logits, int64_t* y, int32_t* rstate,
                              const float* noise, int32_t* stop_idx, float* probs_out, const int32_t* row_seed,
                              const int32_t* row_mask, const float* emb, const float* pe, const float* alpha,
                              float x_scale, float* x, int32_t B, int32_t E, int32_t npos, int32_t dpos, void* stream) {
  return launch_sample_embed_rows(kRows, p, nullptr, logits, y, rstate, noise, stop_idx, probs_out, row_seed, row_mask,
                                  emb, pe, alpha, x_scale, x, nullptr, B, E, npos, dpos, stream);
}

int evt_dec_sample_embed_rows_p(const evt_sample_params* p, const evt_row_sample* row_sample, const float* logits,
                                int64_t* y, int32_t* rstate, const float* noise, int32_t* stop_idx, float* probs_out,
                                const int32_t* row_seed, const int32_t* row_mask, const float* emb, const float* pe,
                                const float* alpha, float x_scale, float* x, int32_t B, int32_t E, int32_t npos,
                                int32_t dpos, void* stream) {
  return launch_sample_embed_rows(kRowsP, p, row_sample, logits, y, rstate, noise, stop_idx, probs_out, row_seed,
                                  row_mask, emb, pe, alpha, x_scale, x, nullptr, B, E, npos, dpos, stream);
}

int evt_dec_sample_embed_rows_lp(const evt_sample_params* p, const evt_row_sample* row_sample, const float* logits,
                                 int64_t* y, int32_t* rstate, const float* noise, int32_t* stop_idx, float* probs_out,
                                 const int32_t* row_seed, const int32_t* row_mask, const float* emb, const float* pe,
                                 const float* alpha, float x_scale, float* x, float* row_logp, int32_t B, int32_t E,
                                 int32_t npos, int32_t dpos, void* stream) {
  return launch_sample_embed_rows(kRowsLp, p, row_sample, logits, y, rstate, noise, stop_idx, probs_out, row_seed,
                                  row_mask, emb, pe, alpha, x_scale, x, row_logp, B, E, npos, dpos, stream);
}

int evt_dec_sample_embed_rows_f(const evt_sample_params* p, const evt_row_sample* row_sample, const float* logits,
                                int64_t* y, int32_t* rstate, const float* noise, int32_t* stop_idx, float* probs_out,
                                const int32_t* row_seed, const int32_t* row_mask, const float* emb, const float* pe,
                                const float* alpha, float x_scale, float* x, float* row_logp, int32_t B, int32_t E,
                                int32_t npos, int32_t dpos, void* stream) {
  return launch_sample_embed_rows(kRowsF, p, row_sample, logits, y, rstate, noise, stop_idx, probs_out, row_seed,
                                  row_mask, emb, pe, alpha, x_scale, x, row_logp, B, E, npos, dpos, stream);
}

}  // extern "C"

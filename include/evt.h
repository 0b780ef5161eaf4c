/*
 * evt.h — C ABI of libevt_hip.so, the MI355X (gfx950) compute library behind the
 * GPT-SoVITS training hot path of megaease/easevoice-trainer.
 *
 * The reference has NO native code: every entry point below replaces a vendor kernel that
 * the reference reaches through torch (ATen / cuDNN / cuBLAS / cuFFT) at the cited call
 * site.  Citations are file:line under /root/reference.
 *
 * Conventions
 *   - plain C, raw device pointers, sizes as int32/int64, `stream` is a hipStream_t passed
 *     as void*; no torch types, no hidden allocation, no global mutable state; every call
 *     only enqueues work on `stream` and returns 0 or a positive errno-style code.
 *   - activations are CHANNELS-LAST: a "sequence tensor" is [nseq][len][channels] with the
 *     channel index contiguous (the reference's [B, C, L] transposed); 16-bit tensors are raw
 *     uint16 storage.  dtype: 0 = float32, 1 = bfloat16, 2 = float16 (fp32 accumulation everywhere).
 *   - the same sources are built twice: libevt_hip.so serves dtype 0 and 1, libevt_hip_f16.so serves
 *     dtype 0 and 2 (the reference's `fp16_run` autocast type, src/train/sovits.py:459-525); both export
 *     exactly this header; a half code the loaded build does not serve returns ENOTSUP (95).
 *     evt_half_dtype() says which one a loaded library is.
 *   - weight gradients / bias gradients are fp32 and are ACCUMULATED (+=) into the caller's
 *     buffers (atomics), so the caller zeroes them once per optimiser step.
 */
#ifndef EVT_H
#define EVT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations of this header are its exported symbols */
#pragma GCC visibility push(default)

#define EVT_DT_F32 0
#define EVT_DT_BF16 1
#define EVT_DT_F16 2
#define EVT_ACT_NONE 0
#define EVT_ACT_LRELU 1
#define EVT_ACT_TANH 2
#define EVT_IMPL_AUTO 0
#define EVT_IMPL_NAIVE 1 /* direct-form reference kernels (any shape, groups) */
#define EVT_IMPL_IGEMM 2 /* LDS-tiled implicit-GEMM on MFMA */

/* "evt-hip <version> (gfx950) src=<12 hex digits>": the digits are a hash of the sources the library was built from
 * (easevoice_trainer_amd/build.py::source_hash); the Python binding refuses a library whose hash differs from the
 * sources next to it. */
const char* evt_version(void);
/* the 16-bit dtype code this build serves: EVT_DT_BF16 (libevt_hip.so) or EVT_DT_F16 (libevt_hip_f16.so) */
int32_t evt_half_dtype(void);
/* Profiling aid, OUTSIDE the contract above and off by default: after evt_debug_kernel_tags(1) every dispatcher
 * records the name of the kernel instantiation it launched in a per-thread buffer that evt_last_kernel_tag() returns
 * (bench.py's roofline leg groups its timings by these names, the same names rocprofv3 prints).  With tags off (the
 * product path) nothing is recorded.  evt_debug_kernel_tags is the library's ONLY process-global mutable state (one flag and
 * a thread-local name buffer): a measurement switch, never read by a computation's arithmetic.  DEBUG ONLY, NOT REENTRANT:
 * switching it while another thread is inside the library is undefined; the product path never calls it. */
void evt_debug_kernel_tags(int32_t enable);
const char* evt_last_kernel_tag(void);

/* Scratch memory the caller must provide, in bytes, for the ops that take a workspace pointer; -1 for an unknown op or
 * a wrong dims count.  The library never allocates.
 *   EVT_WS_MEL          dims = {nseq, wav_len, n_fft, hop, n_mels}   ws of evt_mel_fwd / evt_mel_bwd
 *   EVT_WS_ATTN_BWD     dims = {B, H, L}                             delta_ws of evt_attn_prefixlm_bwd
 *   EVT_WS_MHA_BWD      dims = {B, H, Tq}                            delta_ws of evt_mha_bwd
 *   EVT_WS_MASKED_KL    dims = {}                                    out2 of evt_masked_kl_fwd (sum, live frames)
 *   EVT_WS_NONE         every other entry point: 0 */
#define EVT_WS_NONE 0
#define EVT_WS_MEL 1
#define EVT_WS_ATTN_BWD 2
#define EVT_WS_MHA_BWD 3
#define EVT_WS_MASKED_KL 4
int64_t evt_workspace_bytes(int32_t op, const int64_t* dims, int32_t ndims);

/* ---------------------------------------------------------------------------------------
 * Conv1d / ConvTranspose1d family.
 * Replaces F.conv1d / F.conv_transpose1d / F.conv2d((k,1)) reached from
 *   HiFi-GAN Generator + ResBlock1   src/easevoice/module/models.py:452-471, modules.py:298-311
 *   WN (enc_q, flow)                 src/easevoice/module/modules.py:187-212
 *   FFN convs                        src/easevoice/module/attentions.py:408-416
 *   DiscriminatorS / DiscriminatorP  src/easevoice/module/models.py:538-587
 * One fused op computes, per output position:
 *     y = act_out( conv( lrelu(x, in_slope) ) + bias ) * 1 + res
 * DiscriminatorP's Conv2d (k,1)/(s,1) over [B,1,T/p,p] is the same op on B*p sequences
 * (the caller lays the period axis out as the sequence axis).
 * ------------------------------------------------------------------------------------- */
typedef struct evt_conv1d_params {
  int32_t dtype;      /* EVT_DT_*: activations and prepared weights */
  int32_t nseq;       /* sequences (batch, or batch*period) */
  int32_t lin;        /* input length per sequence */
  int32_t cin, cout;  /* module in/out channels (ConvTranspose: in = weight dim 0) */
  int32_t k, stride, pad, dil, groups;
  int32_t transposed; /* 0 Conv1d (weight [cout][cin/g][k]); 1 ConvTranspose1d (weight [cin][cout][k]) */
  float in_slope;     /* leaky-relu slope applied to x on load; 1.0f = identity */
  int32_t out_act;    /* EVT_ACT_* applied to conv+bias */
  float out_slope;    /* slope when out_act == EVT_ACT_LRELU */
  int32_t impl;       /* EVT_IMPL_* */
} evt_conv1d_params;

/* output length for these hyper-parameters (torch semantics) */
/* 1 when the backward of this conv runs on the LDS-DMA GEMM path (conv_deep), which takes dy with the output
 * activation's derivative already applied (evt_dact_mul) and out_act = EVT_ACT_NONE in the backward calls; else 0. */
int32_t evt_conv1d_wants_plain_dy(const evt_conv1d_params* c);

/* 1 when the FORWARD of this conv (in_slope != 1: leaky-relu on load, the HiFi-GAN upsamplers of models.py:457-460) would
 * run on the LDS-DMA GEMM path if it were handed the activated input: the caller then applies evt_leaky_relu once,
 * calls forward and weight gradient with in_slope = 1 on the activated tensor, and backward-data with in_slope and the
 * activated tensor as `x` (leaky-relu keeps the sign, the derivative is the same).  Else 0. */
int32_t evt_conv1d_wants_plain_x(const evt_conv1d_params* c);

int32_t evt_conv1d_lout(const evt_conv1d_params* p);

/* Prepared-weight layouts.  The parameter tensor is W[d0][d1][k] (Conv1d: d0=cout, d1=cin/g;
 * ConvTranspose1d: d0=cin, d1=cout).  Two GEMM-ready images are derived from it:
 *   REG: [d0][chunk(d1)][k'][ck]                — "rows = d0"; Conv1d forward, ConvT backward-data, all dW
 *   ALT: stride==1: [d1][chunk(d0)][k' flipped][ck]; stride>1: polyphase [phase][d1][chunk(d0)][j][ck]
 *                                                — Conv1d backward-data, ConvT forward
 * evt_conv1d_layout fills the geometry; element counts are in elements of the compute dtype
 * (REG/ALT) or fp32 (dW, same geometry as REG). */
typedef struct evt_wlayout {
  int32_t d0, d1, k, stride;
  int32_t reg_ck, reg_nchunk, reg_kp;          /* REG image */
  int32_t alt_ck, alt_nchunk, alt_kp, alt_nphase; /* ALT image (alt_kp = taps per phase) */
  int64_t reg_elems, alt_elems;
} evt_wlayout;
int evt_conv1d_layout(const evt_conv1d_params* p, evt_wlayout* out);

/* Multi-tensor weight preparation: one launch for a whole model.
 * Replaces torch.nn.utils.weight_norm's per-forward w = g * v / ||v|| (dims 1,2 per d0 row;
 * modules.py:162,174,184,228-296, models.py:427-436,486-536,563-574) plus the cast/layout
 * change into REG and ALT images.  `g` may be NULL for plain (non weight-normed) convs. */
typedef struct evt_wprep_item {
  const float* v;   /* [d0][d1][k] fp32 master (weight_v, or weight when g == NULL) */
  const float* g;   /* [d0] fp32 weight_g or NULL */
  void* reg;        /* REG image (compute dtype) or NULL */
  void* alt;        /* ALT image (compute dtype) or NULL */
  /* backward side (evt_wn_grad_multi): */
  const float* dw;  /* fp32 REG-geometry gradient, accumulated by evt_conv1d_bwd_weight */
  float* dv;        /* [d0][d1][k] fp32, += */
  float* dg;        /* [d0] fp32, += (NULL when g == NULL) */
  evt_wlayout lay;
  int32_t dtype;
  int32_t src_d1;   /* 0, or the parameter's own d1 when lay.d1 was padded up (enc_q.pre: 1025 spectrogram bins in an image
                     * of 1088 columns); v / dv rows then hold src_d1 * k values, the image's extra columns stay zero */
  /* slabs of a deterministic split-K weight gradient (evt_conv1d_bwd_weight_parts); all NULL / 0 without them */
  const float* dw_extra;   /* slabs 1.. of the gradient image, dw_part_stride floats apart (slab 0 is dw) */
  int64_t dw_part_stride;
  const float* db_part;    /* [slab][d0] partial bias gradients or NULL */
  float* db;               /* [d0] fp32 bias gradient, += sum of the db_part slabs in use */
  const int32_t* used;     /* DEVICE int32[2] = {slabs of dw in use (0 or 1: dw only), slabs of db_part in use}: written
                            * by the weight-gradient kernels, reset to 0 by the caller together with dw */
} evt_wprep_item;
/* items is a DEVICE pointer to n items; row_index is a DEVICE int32 [nrows][2] table of
 * (item, d0-row) pairs, one workgroup each. */
int evt_wn_fold_multi(const evt_wprep_item* items, const int32_t* row_index, int32_t nrows, void* stream);
/* The same fold over GROUPS of up to eight consecutive d0-rows of one item: group_index is a DEVICE int32 [ngroups][3] table
 * of (item, first d0-row, rows in the group <= 8), one workgroup each.  A full group of a 16-bit image pair leaves as
 * 16-byte pieces (csrc/elementwise.hip: wn_fold8_kernel); the images are bit-identical to evt_wn_fold_multi's. */
int evt_wn_fold_groups(const evt_wprep_item* items, const int32_t* group_index, int32_t ngroups, void* stream);
int evt_wn_grad_multi(const evt_wprep_item* items, const int32_t* row_index, int32_t nrows, void* stream);

/* y[nseq][lout][cout] = act_out(conv(lrelu(x)) + bias) + res ; bias/res may be NULL.
 * The MFMA path reads REG for Conv1d and ALT for ConvTranspose1d; the direct path reads REG.
 * Pass both images (either may be NULL if the path that needs it cannot be selected). */
int evt_conv1d_fwd(const evt_conv1d_params* p, const void* x, const void* w_reg, const void* w_alt,
                   const float* bias, const void* res, void* y, void* stream);

/* dx[nseq][lin][cin] = convT( dy * act_out'(y) ) * lrelu'(x) + dx_add
 * y may be NULL when out_act == NONE; x may be NULL when in_slope == 1; dx_add may be NULL.
 * The MFMA path reads ALT for Conv1d and REG for ConvTranspose1d; the direct path reads REG. */
int evt_conv1d_bwd_data(const evt_conv1d_params* p, const void* dy, const void* y, const void* w_reg,
                        const void* w_alt, const void* x, const void* dx_add, void* dx, void* stream);

/* dW(REG geometry, fp32) += ..., dbias[cout] += sum(dy * act_out'(y)); dbias may be NULL. */
int evt_conv1d_bwd_weight(const evt_conv1d_params* p, const void* x, const void* dy, const void* y,
                          float* dw, float* dbias, void* stream);

/* The same gradient with a DETERMINISTIC split over the positions.  The MFMA weight-gradient kernels split the
 * reduction over several blocks per output tile; evt_conv1d_bwd_weight combines their partial tiles with fp32 atomics
 * (sum order = finishing order of the blocks: last bits differ from run to run, and every partial tile crosses the
 * fabric as atomic packets).  Here split s owns SLAB s of the gradient image -- slab 0 is `dw` itself, slabs
 * 1 .. parts-1 are dw_extra + (s-1) * part_stride -- and writes it with plain stores: added to slabs that already hold sums of this
 * step (slab 0 when dirty0, slabs below prev_used), stored to the others.  The fused bias gradient goes to db_part[s][cout] the same way (when db_part is NULL: atomics into
 * dbias as before).  evt_wn_grad_multi adds the slabs in index order.  The kernel records the slab counts in
 * used_dev[0..1]; `used` returns the count on the host for the next launch's prev_used.  used == 0 on return: the
 * kernel that handled this shape has no slab mode and accumulated into dw / dbias the classic way.
 * torch.autograd accumulates weight gradients in one fixed order per op; this restores that property. */
typedef struct evt_wgrad_parts {
  float* dw_extra;
  int64_t part_stride;   /* floats */
  float* db_part;
  int32_t* used_dev;
  int32_t parts;         /* slabs provided (>= 1) = upper bound of the split */
  int32_t prev_used;     /* in: slabs already holding partial sums since the last reset (0: none) */
  int32_t used;          /* out */
  int32_t dirty0;        /* in: 1 when slab 0 (dw) may already hold sums of this step -- an earlier launch of any kind since
                          * the caller zeroed it -- and has to be added to; 0: slab 0 is stored like the others (no read) */
  float* ws;             /* scratch (or NULL) for the kernels whose result is tiny -- the Cout = 1 / Cin = 1 layers, the 16-
                          * and 32-channel vocoder stages: their blocks store partial results here and a second launch adds
                          * them into dw / dbias in a fixed order, instead of one fp32 atomic per block and address.  Any
                          * size >= 1 MiB helps (the kernels bound their block count by it); contents need not survive
                          * the call; one buffer per stream. */
  int64_t ws_floats;
} evt_wgrad_parts;
int evt_conv1d_bwd_weight_parts(const evt_conv1d_params* p, const void* x, const void* dy, const void* y,
                                float* dw, float* dbias, evt_wgrad_parts* sp, void* stream);

/* Weight gradients of n convolutions that are ready TOGETHER (the layers of a WN stack, the convolutions of a vocoder
 * stage), declared as a group by the module that owns them.  A convolution launched alone has to fill the chip from the
 * split over its positions, and every split is one more slab of its gradient image written and folded; a group fills it
 * with the tiles of its members, so each member needs fewer splits.  Every member is routed exactly as
 * evt_conv1d_bwd_weight_parts would route it alone (same kernel, same template instantiation); the members that meet in
 * one instantiation of wgrad_ring are launched together, up to EVT_WGRAD_GROUP_MAX per launch (their records travel by
 * value in the kernel arguments), with the split of evt_wgrad_group_plan; every other member goes through
 * evt_conv1d_bwd_weight_parts, in member order.  A launch that ends up with one member is the single launch.  No two
 * members may share a gradient image (EVT_EINVAL).  sp (may be NULL: fp32 atomics) as in evt_conv1d_bwd_weight_parts; its
 * `used` is returned per member. */
#define EVT_WGRAD_GROUP_MAX 16
typedef struct evt_wgrad_member {
  const evt_conv1d_params* p;
  const void* x;
  const void* dy;
  const void* y;
  float* dw;
  float* dbias;
  evt_wgrad_parts* sp;
} evt_wgrad_member;
int evt_conv1d_bwd_weight_group(const evt_wgrad_member* members, int32_t n, void* stream);

/* The split policy of a grouped launch, on the host alone (no device, no pointers, no stream).  members[0..n) are the
 * members of ONE kernel instantiation in the order they were declared; member i goes to launch i / EVT_WGRAD_GROUP_MAX.
 * Per launch: split = ceil(target / tiles of all its members), and per member clamped to
 * [1, min(parts, stages / min_stages)] (parts <= 0: no slabs, no bound from them); per = ceil(stages / split) and
 * nsplit = ceil(stages / per), so every split owns at least one stage.  `target` is the block count the kernel's single
 * launcher aims at.  With n == 1 this is what the single launcher computes. */
typedef struct evt_wgrad_plan {
  int64_t tiles;        /* in: output tiles of the member */
  int32_t stages;       /* in: K stages of its reduction */
  int32_t min_stages;   /* in: fewest stages a split should own */
  int32_t parts;        /* in: slabs provided */
  int32_t launch;       /* out */
  int32_t nsplit;       /* out */
  int32_t per;          /* out: stages per split */
} evt_wgrad_plan;
int evt_wgrad_group_plan(evt_wgrad_plan* members, int32_t n, int64_t target);

/* One HiFi-GAN ResBlock1 step  y = x + c2(lrelu(c1(lrelu(x), dilation d)))  (modules.py:299-308 of the reference; both
 * convolutions C -> C, kernel k, "same" padding, c2 undilated) as ONE launch for the narrow vocoder stages: bf16,
 * C in {16, 32}, k in {3, 7, 11}, d in 1..5.  x, y, xa, mid_a: [nseq][L][C]; w1_reg / w2_reg: the REG images of the two
 * convolutions; b1 / b2 fp32 [C] or NULL.  xa = lrelu(x) and mid_a = lrelu(c1(xa) + b1) are the operands the backward
 * launches (evt_conv1d_bwd_*) take; pass NULL to skip writing them (inference). */
typedef struct evt_resunit_params {
  int32_t dtype, nseq, L, C, k, dil;
  float slope;
} evt_resunit_params;
int32_t evt_resunit_supported(const evt_resunit_params* p);
int evt_resunit_fwd(const evt_resunit_params* p, const void* x, const void* w1_reg, const void* w2_reg, const float* b1,
                    const float* b2, void* xa, void* mid_a, void* y, void* stream);

/* The same step of up to THREE ResBlocks at once -- the three kernel sizes of a HiFi-GAN stage (models.py:457-466:
 * resblock_kernel_sizes 3 / 7 / 11 run side by side on the same input and are averaged) -- as ONE launch: one job per
 * kernel size, all with the same C; each job is what evt_resunit_fwd takes. */
typedef struct evt_resunit_fwd_job {
  evt_resunit_params p;
  const void* x; const void* w1_reg; const void* w2_reg; const float* b1; const float* b2;
  void* xa; void* mid_a; void* y;
} evt_resunit_fwd_job;
int evt_resunit_fwd_multi(const evt_resunit_fwd_job* jobs, int32_t njobs, void* stream);

/* evt_resunit_fwd_multi for a RAGGED batch (inference): row s is live on positions [0, Ls), Ls = min(L, lens[s] * mul),
 * and stored with stride L as before; lens: device int32 [nseq], shared by the jobs (which therefore have one nseq and
 * L); mul: samples of this stage per unit of lens (lens in frames, mul = the product of the up-sampling rates so far).
 * x at positions >= Ls reads as zero whatever the memory holds, the intermediate is zero there (c2's padding), y on
 * [Ls, L) is STORED as zero, xa / mid_a (may be NULL) are written on the live part only.  Tiles start at the row's
 * position 0, so a live output is bit for bit what the one-row launch with L = Ls gives. */
int evt_resunit_fwd_multi_lens(const evt_resunit_fwd_job* jobs, int32_t njobs, const int32_t* lens, int32_t mul,
                               void* stream);

/* The whole backward of the same step in ONE launch (what torch.autograd runs as two conv backward-data, two conv
 * backward-weight and two bias reductions for modules.py:299-308):
 *   dmid = (c2^T dy') * lrelu'(mid_a),  dx = (c1^T dmid) * lrelu'(xa) + dy',  dy' = dy * dy_scale (rounded to bf16: the
 *   1 / num_kernels of the stage mean, models.py:466, folded into the load; 1.0 = plain dy),
 *   dw2 += dy' (x) mid_a, dw1 += dmid (x) xa (fp32 gradient images, REG geometry), db2 += sum dy', db1 += sum dmid.
 * w1_alt / w2_alt: the ALT images of the two convolutions.  dmid (optional, may be NULL): receives dmid [nseq][L][C].
 * Weight gradients: evt_resunit_bwd_supported(p, 1) says whether the launch can accumulate them (not for C = 32 with
 * 11 taps: the two images do not fit the register file); then dw1, dw2 != NULL and ws = scratch of at least
 * evt_resunit_bwd_ws_floats() floats (one buffer per stream, contents need not survive the call): blocks store partial
 * gradient rows there and a second launch adds them in block order -- the result does not depend on timing.  Otherwise
 * pass dw1 == dw2 == NULL and dmid != NULL and run evt_conv1d_bwd_weight(xa, dmid) / (mid_a, dy) for the two gradients.
 * db1 / db2 may be NULL.  evt_resunit_bwd_multi: one to three jobs (one per kernel size 3 / 7 / 11, same C) in one
 * launch, each job as described. */
int32_t evt_resunit_bwd_supported(const evt_resunit_params* p, int32_t with_weight_grads);
int64_t evt_resunit_bwd_ws_floats(const evt_resunit_params* p);
int evt_resunit_bwd(const evt_resunit_params* p, const void* dy, float dy_scale, const void* xa, const void* mid_a,
                    const void* w1_alt, const void* w2_alt, void* dx, void* dmid, float* dw1, float* dw2, float* db1,
                    float* db2, float* ws, int64_t ws_floats, void* stream);
typedef struct evt_resunit_bwd_job {
  evt_resunit_params p;
  float dy_scale;
  const void* dy; const void* xa; const void* mid_a; const void* w1_alt; const void* w2_alt;
  void* dx; void* dmid;
  float* dw1; float* dw2; float* db1; float* db2;
} evt_resunit_bwd_job;
int evt_resunit_bwd_multi(const evt_resunit_bwd_job* jobs, int32_t njobs, float* ws, int64_t ws_floats, void* stream);

/* The same step for the WIDE vocoder stages (bf16, C in {64, 128}, k in {3, 7, 11}, d in 1..5) with the activated
 * intermediate kept in LDS: forward in one launch (instead of leaky-relu + two convolutions), and the DATA half of the
 * backward in one launch -- dmid = (c2^T dy') * lrelu'(mid_a) and dx = (c1^T dmid) * lrelu'(xa) + dy', dy' = dy * dy_scale
 * rounded to bf16 -- instead of two.  dmid [nseq][L][C] is written for the two weight-gradient launches
 * (evt_conv1d_bwd_weight on (mid_a, dy') and (xa, dmid)), which stay separate: at these widths a gradient image does not
 * fit a wave's registers.  Operands as in evt_resunit_fwd / evt_resunit_bwd. */
int32_t evt_resunit_wide_supported(const evt_resunit_params* p);
int evt_resunit_wide_fwd(const evt_resunit_params* p, const void* x, const void* w1_reg, const void* w2_reg, const float* b1,
                         const float* b2, void* xa, void* mid_a, void* y, void* stream);
/* evt_resunit_wide_fwd for a ragged batch: lens / mul and the treatment of x, the intermediate, y, xa and mid_a (both may
 * be NULL) as in evt_resunit_fwd_multi_lens. */
int evt_resunit_wide_fwd_lens(const evt_resunit_params* p, const void* x, const void* w1_reg, const void* w2_reg,
                              const float* b1, const float* b2, void* xa, void* mid_a, void* y, const int32_t* lens,
                              int32_t mul, void* stream);
int evt_resunit_wide_bwd_data(const evt_resunit_params* p, const void* dy, float dy_scale, const void* xa, const void* mid_a,
                              const void* w1_alt, const void* w2_alt, void* dmid, void* dx, void* stream);

/* One layer of the WN stack of the posterior encoder / the flow (modules.py:187-211 of the reference) FORWARD in one launch
 * (16-bit type, H = 192, k = 5, dilation 1): x_in = in_layer(x) [nseq][L][2H], acts = tanh(x_in[:H] + g[:H]) *
 * sigmoid(x_in[H:] + g[H:]) [nseq][L][H], rs = res_skip(acts); x_out = (x + rs[:H]) * mask, acc_out = acc_in + rs[H:]
 * (last != 0: res_skip has H outputs, acc_out = (acc_in + rs) * mask, x_out unused).  Replaces evt_conv1d_fwd +
 * evt_gated_act_fwd + evt_conv1d_fwd + evt_wn_residual_fwd with the same rounding points (x_in, acts, rs rounded to the
 * 16-bit type); the gate output stays in LDS between the two convolutions.  w_in_frag / w_rs_frag: the two convolutions'
 * REG images (evt_conv1d_layout) re-ordered by evt_frag_pack, b_in [2H] / b_rs [2H or H] fp32 or NULL, g [nseq][2H] or
 * NULL, acc_in NULL for the first layer, lens [nseq] or NULL (mask = position < lens[sequence]).  x_in and acts are outputs
 * the backward launches (evt_gated_act_bwd, the weight gradients) read, as before.  EVT_ENOTSUP outside that shape family.
 *
 * evt_frag_pack: items is a DEVICE table; each item copies a REG or ALT image of `rows` (multiple of 16) rows x `ktot`
 * (multiple of 32) elements of the 16-bit type into FRAGMENT ORDER [rows / 16][ktot / 32][64][8] -- lane (n, g) of (tile, K step)
 * holds row 16 tile + n, elements 32 ks + 8 g .. + 7, i.e. every MFMA A operand is one contiguous 1 KiB load of a wave.
 * One launch per weight fold for all such images of a model (they change when the weights do).  Readers: evt_wn_layer_fwd,
 * evt_wn_layer_bwd_data. */
typedef struct evt_frag_item {
  const void* src;   /* REG or ALT image, [rows][ktot] */
  void* dst;         /* rows * ktot elements */
  int32_t rows, ktot;
} evt_frag_item;
int evt_frag_pack(const evt_frag_item* items, int32_t nitems, void* stream);
/* evt_wn_layer_bwd_data: the data half of the same layer's backward in one launch (instead of evt_wn_residual_bwd, the 1 x 1
 * evt_conv1d_bwd_data, evt_gated_act_bwd and the k = 5 evt_conv1d_bwd_data with its add epilogue):
 *   drs = [dx_next * mask | dacc] [nseq][L][2H]   (last: drs = dacc * mask [nseq][L][H]; dx_next must be NULL)
 *   dacts = res_skip^T drs;  dx_in = gate'(x_in + g) dacts [nseq][L][2H];  dg [nseq][2H] fp32 += sum over positions (or NULL)
 *   dx = in_layer^T dx_in + dx_next * mask [nseq][L][H]
 * w_rs_alt_frag / w_in_alt_frag: the ALT images in fragment order.  drs and dx_in are outputs the two weight-gradient
 * launches (evt_conv1d_bwd_weight on (acts, drs) and (x, dx_in)) read, as before. */
int evt_wn_layer_bwd_data(int32_t dtype, const void* dx_next, const void* dacc, const void* x_in, const void* g,
                          const void* w_rs_alt_frag, const void* w_in_alt_frag, const int32_t* lens, void* drs, void* dx_in,
                          void* dx, float* dg, int32_t nseq, int32_t L, int32_t H, int32_t k, int32_t last, void* stream);
int32_t evt_wn_layer_supported(int32_t dtype, int32_t H, int32_t k, int32_t dil);
int evt_wn_layer_fwd(int32_t dtype, const void* x, const void* w_in_frag, const float* b_in, const void* w_rs_frag,
                     const float* b_rs, const void* g, const void* acc_in, const int32_t* lens, void* x_in, void* acts,
                     void* x_out, void* acc_out, int32_t nseq, int32_t L, int32_t H, int32_t k, int32_t last, void* stream);

/* ---------------------------------------------------------------------------------------
 * Element-wise / reduction helpers of the s2 path.
 * ------------------------------------------------------------------------------------- */
/* out = (a + b + c) * scale ; b, c may be NULL.  (Generator stage mean, models.py:457-466) */
int evt_add3_scale(int32_t dtype, const void* a, const void* b, const void* c, float scale, void* out,
                   int64_t n, void* stream);

/* x[s][t][:] = 0 for t >= lens[s] * mul, in place; x [nseq][L][C], lens device int32 [nseq].  The dead tails of a ragged
 * batch in front of a consumer that has no masked load (the vocoder's first up-sampler, the unfused ResBlock steps).
 * C * element size a multiple of 16, x 16-byte aligned. */
int evt_mask_tail(int32_t dtype, void* x, const int32_t* lens, int32_t mul, int32_t nseq, int32_t L, int32_t C,
                  void* stream);

/* Per-row linear resampling along the positions: the speed change of the prior encoder's output (models.py:246-248,
 * F.interpolate(mode="linear") per sequence) for a RAGGED batch, every row with its own input and output length.
 * x [nseq][Lin][C] -> y [nseq][Lout][C], in_lens / out_lens device int32 [nseq], clamped on the device to [0, Lin] /
 * [0, Lout].  Row s with Ti = in_lens[s], To = out_lens[s], in fp32 (torch's upsample_linear1d, align_corners = False):
 *   scale = (float)Ti / (float)To;  src = max(scale * (j + 0.5f) - 0.5f, 0);  i0 = (int)src;  i1 = i0 + (i0 < Ti - 1)
 *   l1 = src - i0  (0 where i0 is the row's last position: both taps are that position, y is x there exactly)
 *   y[s][j] = (1 - l1) * x[s][i0] + l1 * x[s][i1]   for j < To,  rounded once to the storage type
 *   y[s][j] = 0                                     for To <= j < Lout (and everywhere when Ti == 0)
 * x is never read at positions >= Ti, every element of y is written (no evt_mask_tail behind it), a row with To == Ti
 * is a copy.  No host synchronisation: legal in a captured graph.  C * element size a multiple of 16, x and y 16-byte
 * aligned; EVT_EINVAL otherwise, and for a NULL pointer, a size <= 0 or a dtype the build does not serve. */
int evt_resample_rows(int32_t dtype, const void* x, const int32_t* in_lens, const int32_t* out_lens, int32_t nseq,
                      int32_t Lin, int32_t Lout, int32_t C, void* y, void* stream);

/* The finishing launch of a ragged decode: every row of a batch of waveforms resampled from in_rate to out_rate
 * (up / down = out_rate / in_rate, reduced), converted to the output format and packed into one buffer with `gap` zeros
 * behind each row -- the int16 conversion and the silence interval of the reference's audio_postprocess
 * (inference/tts.py:878-908) and a resampler in front of them, in one launch.
 *
 * The operator.  rho = 0.9475937167399596, beta = 14.769656459379492, Z = EVT_RESAMPLE_ZEROS (resampy's kaiser_best, the
 * filter of feature_extractor/normalize.py::resample_half, which this is at up / down = 1 / 2); s = min(1, up / down),
 * H = Z * max(up, down).  Prototype filter in float64, for integer |k| < H, zero outside:
 *   g[k] = s * rho * sinc(rho * s * k / up) * I0(beta * sqrt(1 - (s * k / (up * Z))^2)) / I0(beta)   sinc(t) = sin(pi t) / (pi t)
 * A row of n live samples gives To = (n * up) / down outputs (integer division, 64-bit):
 *   y[m] = sum_{i = 0}^{n - 1} x[i] * g[m * down - i * up]        0 <= m < To,   x = 0 outside [0, n)
 * Polyphase form: c = m * down, q = c / up, p = c % up, R = ceil(H / up);  y[m] = sum_j T[p][j] * x[q - R + j] with
 * T[p][j] = g[p + (R - j) * up] for j = 0 .. 2 R and 0 for 2 R < j < J: the caller's `table` [up][J], built in float64 and
 * rounded once to fp32, J a multiple of 4 in [2 R + 1, 2 R + 4], 16-byte aligned.  up == down == 1 is NOT this filter
 * (g[0] = rho) but the identity, table may be NULL then and J is ignored.
 * Arithmetic: x widened to fp32 (exact), products and sums in fp32 in a fixed order that depends on (m, up, down) only:
 * four accumulators a0 .. a3 = 0; for j = 0, 4, 8, ... ascending a_e = fma(T[p][j + e], x[q - R + j + e], a_e), e = 0 .. 3;
 * y[m] = (a0 + a1) + (a2 + a3).  A row therefore comes out bit for bit as it does with nseq = 1.
 *
 * x [nseq][L] of dtype; lens device int32 [nseq], row s has n_s = min(max(lens[s] * mul, 0), L) live samples and x is never
 * read at or behind them.  Row s writes To_s samples at out[out_off[s] ..] and `gap` zeros directly behind them (out_off
 * device int64 [nseq]; with the offsets a prefix sum of To_s + gap every element of `out` is written, no memset in front);
 * an element that would fall outside [0, out_elems) is not stored.  out_format EVT_PCM_F32: the fp32 value v;
 * EVT_PCM_S16: (int16) trunc(min(max(v * 32768, -32768), 32767)), NaN -> 0 (the reference's (audio * 32768).astype(int16),
 * saturating where numpy wraps around).  Lengths are read on the device, no host synchronisation: legal in a captured
 * graph.  A block takes EVT_RESAMPLE_TILE consecutive outputs of one row, counted from the row's output 0.
 * EVT_EINVAL for a NULL pointer, a size <= 0, up or down <= 0, gap < 0, nseq > 65535, a pointer not aligned to its element
 * (table: 16 bytes), a J outside the range above, an unknown format or a dtype the build does not serve. */
#define EVT_RESAMPLE_ZEROS 64
#define EVT_RESAMPLE_TILE 2048
#define EVT_PCM_F32 0
#define EVT_PCM_S16 1
int evt_resample_pack_rows(int32_t dtype, const void* x, const int32_t* lens, int32_t mul, int32_t nseq, int32_t L,
                           int32_t up, int32_t down, const float* table, int32_t J, int32_t out_format, void* out,
                           int64_t out_elems, const int64_t* out_off, int32_t gap, void* stream);

/* The first launch of the audio pipeline: the sample bytes of nrec WAV recordings that share an input rate, decoded, mixed
 * down to mono and resampled to the pipeline's rate (up / down = out_rate / in_rate, reduced) into one packed fp32 buffer
 * -- the batch form of the reference's load_audio (utils/audio/__init__.py:13-32: ffmpeg, ac=1, ar=sr) and of the
 * librosa.load(path, sr=16000) of _set_prompt_semantic (inference/tts.py:411-437), in one launch.  ffmpeg's swr resampler is
 * another filter: at a changed rate the samples are this operator's, not ffmpeg's.
 *
 * raw: raw_len bytes on the device, the recordings' sample bytes (the body of a WAV file's data chunk: interleaved frames,
 * little-endian).  Recording r has frames[r] frames of channels[r] samples in format fmt[r], its first byte at
 * raw[byte_off[r]]; byte_off, frames (int64), fmt, channels (int32) and out_off (int64) are device tables of nrec entries.
 * n_r = min(max(frames[r], 0), max_frames) frames are read; max_frames is the host's upper bound, it sizes the grid.
 *
 * The operator, per recording, with C = channels[r] and W the sample's bytes:
 *   Decode.  Sample s of a frame -> fp32 v, every step exact or ONE round-to-nearest-even (rne_f32):
 *     EVT_PCM_IN_U8  (W = 1, unsigned)                    v = (s - 128) * 2^-7
 *     EVT_PCM_IN_S16 (W = 2, signed)                      v = s * 2^-15
 *     EVT_PCM_IN_S24 (W = 3, signed, sign-extended)       v = s * 2^-23
 *     EVT_PCM_IN_S32 (W = 4, signed)                      v = rne_f32(s) * 2^-31
 *     EVT_PCM_IN_F32 (W = 4, IEEE binary32)               v = the value itself
 *     EVT_PCM_IN_F64 (W = 8, IEEE binary64)               v = rne_f32(value)
 *   NaN and infinities pass through, nothing is clamped.
 *   Downmix.  m[i] = fdiv(((v_0 + v_1) + v_2) + ... + v_{C-1}, (float)C) over the C samples of frame i: the additions in
 *   channel order, each rounded to fp32, the division correctly rounded -- numpy's x.reshape(-1, C).mean(axis=1,
 *   dtype=float32) for C <= 8.  C = 1: m[i] = v_0, bits unchanged.  For a PCM16 file this is train/dataset.py::read_wav_pcm16
 *   bit for bit.
 *   Resample.  The operator of evt_resample_pack_rows above applied to x = m[0 .. n_r), nothing changed: the same table
 *   [up][J], To_r = (n_r * up) / down outputs, the same four accumulators in the same order and (a0 + a1) + (a2 + a3);
 *   up == down == 1 is the identity, table may be NULL then and J is ignored.  A recording therefore comes out bit for bit
 *   as it does alone, and as evt_resample_pack_rows gives for the row m.
 *   Output.  To_r fp32 values at out[out_off[r] ..]; an element that would fall outside [0, out_elems) is not stored.  With
 *   out_off the prefix sum of To_r every element of `out` is written.
 *
 * No byte outside [byte_off[r], byte_off[r] + n_r * C * W) is read for recording r: a sample is read with a load of its own
 * size, or byte by byte, never with a wider one.  A recording whose bytes do not lie inside [0, raw_len), whose fmt is not
 * one of the six codes or whose channels lie outside 1 .. EVT_PCM_IN_MAX_CHANNELS is skipped on the device: its outputs are
 * not written.  byte_off needs no alignment (an aligned recording is read with fewer loads).  A block takes
 * EVT_RESAMPLE_TILE consecutive outputs of one recording, counted from its output 0; format and channel count are
 * block-uniform.  No host synchronisation and no 16-bit type: the same code in both builds.
 * EVT_EINVAL (nothing launched) for a NULL pointer, raw_len, nrec, max_frames or out_elems <= 0, nrec > 65535, max_frames
 * >= 2^31, up or down <= 0, a J outside the range of evt_resample_pack_rows, a table not 16-byte aligned or a table or
 * `out` not aligned to its element.  EVT_OK without a launch when (max_frames * up) / down == 0: no recording has an output. */
#define EVT_PCM_IN_U8 0
#define EVT_PCM_IN_S16 1
#define EVT_PCM_IN_S24 2
#define EVT_PCM_IN_S32 3
#define EVT_PCM_IN_F32 4
#define EVT_PCM_IN_F64 5
#define EVT_PCM_IN_MAX_CHANNELS 8
int evt_pcm_ingest_rows(const uint8_t* raw, int64_t raw_len, const int64_t* byte_off, const int64_t* frames,
                        const int32_t* fmt, const int32_t* channels, int32_t nrec, int64_t max_frames, int32_t up,
                        int32_t down, const float* table, int32_t J, float* out, int64_t out_elems, const int64_t* out_off,
                        void* stream);

/* out = leaky_relu(x, slope).  The HiFi-GAN residual unit (modules.py:299-308) keeps an activated copy of its input
 * so that its convolutions and weight gradients take plain operands (LDS-DMA kernels).  16-byte aligned. */
int evt_leaky_relu(int32_t dtype, const void* x, float slope, void* out, int64_t n, void* stream);

/* out = dy * act'(y), the activation derivative taken through the activation OUTPUT y (leaky-relu keeps the sign,
 * tanh' = 1 - y^2).  Replaces the autograd node of F.leaky_relu after a wide DiscriminatorP conv
 * (models.py:527-531) when evt_conv1d_wants_plain_dy() says the GEMM-grade path will consume dy: both backward
 * GEMMs then read the pre-multiplied tensor instead of fusing the derivative into their loads.  16-byte aligned. */
int evt_dact_mul(int32_t dtype, const void* dy, const void* y, int32_t act_kind, float slope, void* out, int64_t n,
                 void* stream);

/* WN gated activation, commons.py:94-101 (fused_add_tanh_sigmoid_multiply), channels-last:
 *   acts[n][t][h] = tanh(xin[n][t][h] + g[n][h]) * sigmoid(xin[n][t][H+h] + g[n][H+h])
 * g is [nseq][2H] (broadcast over t) or NULL. */
int evt_gated_act_fwd(int32_t dtype, const void* xin, const void* g, void* acts, int32_t nseq, int32_t len,
                      int32_t H, void* stream);
/* dxin = d(acts)/d(xin) * dacts ; dg[nseq][2H] (fp32, +=) may be NULL */
int evt_gated_act_bwd(int32_t dtype, const void* xin, const void* g, const void* dacts, void* dxin, float* dg,
                      int32_t nseq, int32_t len, int32_t H, void* stream);


/* STFT magnitude + mel + log of the generated waveform, src/easevoice/module/mel_processing.py:93-142:
 * reflect-pad (n_fft-hop)/2, hann window, n_fft-point real DFT per frame (radix-2 in LDS, wavefront
 * shuffles for the short butterflies), sqrt(re^2+im^2+1e-6), mel basis [n_mels][n_fft/2+1] matmul,
 * log(clamp(.,1e-5)).  wav is fp32 [nseq][wav_len]; outputs fp32 channels-FIRST [nseq][n_mels][frames]
 * (the layout the mel-L1 at sovits.py:513 consumes).  spec_out ([nseq][n_fft/2+1][frames]) may be NULL. */
int evt_mel_fwd(const float* wav, const float* window, const float* mel_basis, float* spec_out, float* mel_out,
                float* ws_spec_re_im, int32_t nseq, int32_t wav_len, int32_t n_fft, int32_t hop, int32_t n_mels,
                void* stream);
/* dwav[nseq][wav_len] = d(sum(dmel * mel))/d(wav); ws is the (re,im,mag,melpre) workspace written by fwd. */
int evt_mel_bwd(const float* dmel, const float* window, const float* mel_basis, const float* ws_spec_re_im,
                float* dwav, int32_t nseq, int32_t wav_len, int32_t n_fft, int32_t hop, int32_t n_mels, void* stream);
/* workspace floats needed by evt_mel_fwd/bwd; 0 for hop <= 0 (which they refuse) */
int64_t evt_mel_workspace_floats(int32_t nseq, int32_t wav_len, int32_t n_fft, int32_t hop, int32_t n_mels);

/* Linear spectrograms of a RAGGED batch of reference clips: the reference's _get_ref_spec (inference/tts.py:390-409: peak,
 * audio /= min(2, peak) where the peak exceeds 1, spectrogram_torch) for nseq clips at once, the FFT arithmetic of evt_mel_fwd.
 *   x fp32 [nseq][N]; lens device int32 [nseq], row s has n_s = min(max(lens[s], 0), N) live samples and x is never read at or
 *   behind them; window fp32 [n_fft]; n_fft = 2048; pad = (n_fft - hop) / 2.
 *   Row s has F_s = (n_s + 2 pad - n_fft) / hop + 1 frames when n_s > pad and n_s + 2 pad >= n_fft, else 0 (n_s / 640 at hop
 *   640); Fmax is the same count for n_s = N.
 * Two launches on `stream`, no host synchronisation: legal in a captured graph.
 *   peak[s] = max_{i < n_s} |x[s][i]|   (fp32 [nseq], an OUTPUT; NaN if the live part holds a NaN, 0 for an empty row)
 *   v[i]    = peak[s] > 1 ? fdiv(x[s][i], min(2, peak[s])) : x[s][i]      the division rounded to fp32 on its own
 *   frame f < F_s, sample j < n_fft:  q = f * hop + j - pad;  i = |q| for q < n_s, 2 (n_s - 1) - q from there on: the reflect
 *   padding at the ROW's own ends;  X = DFT_2048(v[i] * window[j]);  out[s][f][k] = sqrt(re_k^2 + im_k^2 + 1e-6), k < bins
 *   out[s][f][:] = 0  for F_s <= f < Fmax
 * out fp32 channels-LAST [nseq][Fmax][bins], 1 <= bins <= n_fft / 2 + 1: only the first `bins` bins are stored (the style
 * encoder takes 704).  Every element of out is written, no memset in front; 16-byte stores where bins is a multiple of 4.
 * One block per (row, frame): neither nseq nor N enters the arithmetic, a row is bit for bit what nseq = 1 gives with any
 * N >= n_s.  N so short that Fmax = 0: peak is written, out has no element.
 * EVT_EINVAL (nothing launched) for a NULL pointer, nseq <= 0 or > 65535, N <= 0, n_fft != 2048, hop <= 0 or > n_fft, bins
 * outside the range above, out not 16-byte aligned. */
int evt_ref_spec_rows(const float* x, const int32_t* lens, int32_t nseq, int32_t N, const float* window, int32_t n_fft,
                      int32_t hop, int32_t bins, float* out, float* peak, void* stream);

/* ---------------------------------------------------------------------------------------
 * Input front-end of the s2 step (no gradients).
 * ------------------------------------------------------------------------------------- */
/* Layout change at the model boundary: src fp32 [B][C][T] (the reference's layout: spectrogram, ssl features) ->
 * dst [B][T][Cp] in `dtype`, channels c >= C written as zeros.  With Cp a multiple of 64 the 1025-bin projection
 * enc_q.pre (models.py:348-352) runs on the library's GEMM kernels (its prepared image is padded to Cp columns). */
int evt_ncl_to_nlc(int32_t dtype, const float* src, void* dst, int32_t B, int32_t C, int32_t T, int32_t Cp, void* stream);

/* Frozen quantizer look-up (models.py:912-926 -> quantize.py:70-94 -> core_vq.py:172-228, n_q = 1, eval):
 *   evt_rvq_norms : ee[k] = |embed[k]|^2                                                   (embed fp32 [K][D])
 *   evt_rvq_select: code[n] = argmax_k -(|h_n|^2 - 2 dots[n][k] + ee[k]), first maximum; q_out rows n*rep .. n*rep+rep-1
 *                   = embed[code[n]]  (rep = 2: the x2 nearest up-sampling of the 25 Hz codes)
 * dots [N][K] = h . embed^T comes from evt_conv1d_fwd (a 1x1 layer whose weight is the codebook), h [N][D] from the
 * ssl_proj convolution, both in fp32 whatever the compute dtype of the step (the reference disables autocast there). */
int evt_rvq_norms(const float* embed, float* ee, int32_t K, int32_t D, void* stream);
int evt_rvq_select(const float* h, const float* dots, const float* embed, const float* ee, int64_t* codes, float* q_out,
                   int32_t N, int32_t D, int32_t K, int32_t rep, void* stream);

/* Target-side mel (mel_processing.py:77-90 + commons.slice_segments at sovits.py:478-480):
 *   out[b][m][f] = log(max(sum_k basis[m][k] * spec[b][k][starts[b] + f], 1e-5)),  f < nfr
 * spec fp32 [B][F][T] (reference layout), basis fp32 [M][F], starts int64 [B] or NULL (= 0), out fp32 [B][M][nfr]. */
int evt_spec_to_mel(const float* spec, const float* basis, const int64_t* starts, float* out, int32_t B, int32_t F,
                    int32_t T, int32_t M, int32_t nfr, void* stream);

/* Fused loss reductions (src/easevoice/module/losses.py:7-61).  Pointer tables are DEVICE arrays.
 * feature_loss: out[0] += 2 * sum_i mean|r_i - g_i| ; optional dg_i = 2*sign(g_i-r_i)/n_i * dloss. */
typedef struct evt_seg { const void* a; const void* b; void* da; int64_t n; float scale; int32_t pad_; } evt_seg;
int evt_l1_multi_fwd(int32_t dtype, const evt_seg* segs, int32_t nseg, float* out, void* stream);
int evt_l1_multi_bwd(int32_t dtype, const evt_seg* segs, int32_t nseg, const float* dloss, void* stream);
/* LSGAN: out[0] += sum_i scale_i * mean((target - a_i)^2) ; da_i = -2*scale_i*(target - a_i)/n_i * dloss */
int evt_lsgan_multi_fwd(int32_t dtype, const evt_seg* segs, int32_t nseg, float target, float* out, void* stream);
int evt_lsgan_multi_bwd(int32_t dtype, const evt_seg* segs, int32_t nseg, float target, const float* dloss,
                        void* stream);

/* Masked KL term of the generator loss, src/easevoice/module/losses.py:46-61:
 *   kl = logs_p - logs_q - 0.5 + 0.5 (z_p - m_p)^2 exp(-2 logs_p);  loss = sum(kl * z_mask) / sum(z_mask)
 * with z_mask[b][t] = (t < lens[b]) (lens NULL = all live).  The four tensors share one layout: [B][T][C] (time_inner
 * = 0, channels-last) or [B][C][T] (time_inner = 1, the reference's); each has its own dtype.
 * fwd: out2[0] += sum(kl * z_mask) (caller zeroes it), out2[1] = sum(z_mask) = live frames; loss = out2[0] / out2[1].
 * bwd: gradients of loss * dloss[0] w.r.t. the four inputs (dtype of the input; any may be NULL), masked positions
 * get zeros; `count` points at out2[1]. */
typedef struct evt_kl_params {
  int32_t B, T, C, time_inner;
  int32_t dt_z_p, dt_logs_q, dt_m_p, dt_logs_p;
} evt_kl_params;
int evt_masked_kl_fwd(const evt_kl_params* p, const void* z_p, const void* logs_q, const void* m_p, const void* logs_p,
                      const int32_t* lens, float* out2, void* stream);
int evt_masked_kl_bwd(const evt_kl_params* p, const void* z_p, const void* logs_q, const void* m_p, const void* logs_p,
                      const int32_t* lens, const float* dloss, const float* count, void* dz_p, void* dlogs_q, void* dm_p,
                      void* dlogs_p, void* stream);

/* Multi-segment AdamW over a flat fp32 arena (torch.optim.AdamW at sovits.py:294-319: decoupled
 * weight decay, bias correction, eps outside the sqrt).  seg table is a DEVICE array (<= 64 segments);
 * elements of [0, n) outside every segment are left untouched (frozen parameters, alignment padding). */
typedef struct evt_adamw_seg { int64_t begin, end; float lr; float weight_decay; } evt_adamw_seg;
int evt_adamw_flat(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   const evt_adamw_seg* segs, int32_t nseg, float beta1, float beta2, float eps, int32_t step,
                   float grad_scale, void* stream);
/* The same update with the step number in DEVICE memory: *step_counter is incremented by one (a 1-thread launch) and
 * the bias corrections are computed from it on the device.  No argument changes from step to step, so the call can be
 * captured into a HIP graph and replayed. */
int evt_adamw_flat_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                       const evt_adamw_seg* segs, int32_t nseg, float beta1, float beta2, float eps,
                       int32_t* step_counter, float grad_scale, void* stream);
/* The same update restricted to the elements [lo, hi) of the arena: lets a step update one sub-model's parameters as soon
 * as its gradients are complete, on a side stream, under the backward of the next sub-model (AdamW is element-wise: the
 * ranges of one step may run in any order and give the bits of the single launch).  bump != 0 increments *step_counter
 * first -- exactly one range call per step passes it, the first one enqueued; all of them must be ordered after it. */
int evt_adamw_flat_dev_range(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t lo, int64_t hi,
                             const evt_adamw_seg* segs, int32_t nseg, float beta1, float beta2, float eps,
                             int32_t* step_counter, int32_t bump, float grad_scale, void* stream);
/* Input side of MultiPeriodDiscriminator (src/easevoice/module/models.py:541-547 DiscriminatorP: reflect-pad to a multiple of
 * the period, view [B, 1, T/p, p]; models.py:576-587 DiscriminatorS: the waveform itself = period 1) for ALL sub-discriminators
 * in one launch.  The waveform batch is [src0 ; src1] (n0 + n1 items of T samples; src1 may be NULL with n1 = 0), for
 * period p_i:   outs[i][(b * p_i + ph)][j][0] = x[b][t],  t = j * p_i + ph,  t >= T mirrored to 2T - 2 - t,
 * outs[i] holding (n0 + n1) * p_i sequences of ceil(T / p_i) positions of one channel, in out_dtype.  nper <= 8; the two
 * sources may differ in dtype (real audio fp32, generated audio in the compute dtype). */
int evt_mpd_fold(int32_t src0_dtype, const void* src0, int32_t n0, int32_t src1_dtype, const void* src1, int32_t n1, int32_t T,
                 const int32_t* periods, int32_t nper, void* const* outs, int32_t out_dtype, void* stream);
/* Its backward: dsrc[b][t] = sum_i (douts[i] at the positions that read x[b0 + b][t], the mirrored tail included), for the
 * n items starting at item b0 of the prepared batches (the generated half of [real ; generated]: b0 = n0). */
int evt_mpd_unfold(int32_t grad_dtype, const void* const* douts, const int32_t* periods, int32_t nper, int32_t b0, int32_t n,
                   int32_t T, int32_t dsrc_dtype, void* dsrc, void* stream);

/* out[0] = sum(x^2) over n floats (grad-norm at commons.py:140-155 without the per-parameter .item()) */
int evt_sumsq(const float* x, int64_t n, float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Loss scaling of the fp16 mode (torch.cuda.amp.GradScaler at src/train/sovits.py:378 and :504-507, :521-525:
 * scale(loss).backward(); unscale_(optim); step(optim); update()), with every piece of state in DEVICE memory so that
 * the step stays free of host synchronisation and can be captured into a HIP graph.
 *   scale [1] fp32, growth_tracker [1] int32, found_inf [1] fp32 per optimiser (0 = all gradients finite).
 * evt_scaler_unscale: grad[i] *= 1 / scale (the reciprocal taken in double and rounded to fp32, as GradScaler._unscale_grads_
 *   does), *found_inf = 1 if any element is inf / NaN (torch._amp_foreach_non_finite_check_and_unscale_); found_inf is only
 *   ever raised here, evt_scaler_update clears it.
 * evt_adamw_flat_dev_guarded: evt_adamw_flat_dev that does NOTHING -- no update, no step-counter increment -- when
 *   *skip != 0 (GradScaler.step skips optimizer.step() on an overflow); skip == NULL: unconditional.
 * evt_scaler_update: torch._amp_update_scale_: any of the nflags <= 4 flags set -> scale *= backoff_factor, tracker = 0;
 *   else tracker += 1 and, when it reaches growth_interval, scale *= growth_factor (kept only if finite), tracker = 0.
 *   The flags are reset to 0 for the next step. */
int evt_scaler_unscale(float* grad, int64_t n, const float* scale, float* found_inf, void* stream);
int evt_adamw_flat_dev_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                               const evt_adamw_seg* segs, int32_t nseg, float beta1, float beta2, float eps,
                               int32_t* step_counter, float grad_scale, const float* skip, void* stream);
int evt_scaler_update(float* scale, int32_t* growth_tracker, float* const* found_inf, int32_t nflags, float growth_factor,
                      float backoff_factor, int32_t growth_interval, void* stream);

/* ---------------------------------------------------------------------------------------
 * s1 (text -> semantic GPT) kernels.
 * ------------------------------------------------------------------------------------- */
/* Dense layers ("gemm_bf16" of SURVEY 8(b)):  y[M][N] = act(x[M][K] . W[N][K]^T + bias),  act = relu when `relu`.
 * Replaces F.linear at transformer.py:207-224,330-334 (linear1 / linear2), patched_mha_with_cache.py:242,460 (packed
 * in-projection, out-projection) and t2s_model.py:276,486 (bert_proj, ar_predict_layer).  dtype EVT_DT_BF16 runs on the
 * LDS-DMA MFMA kernels (fp32 accumulation), EVT_DT_F32 is the fp32-MFMA parity path.  K % 8 == 0 and N % 8 == 0 (a
 * caller with an odd N, e.g. the 1025-entry vocabulary, pads the weight image and the output to a multiple of 128 with
 * zero rows / columns).
 * The weights are passed as the two prepared images of evt_gemm_bf16_layout (same structs as the convolutions:
 * evt_wn_fold_multi with g == NULL casts an fp32 master into both images in one launch for all layers):
 *   REG = W row-major [N][K] in chunks of reg_ck (forward, dW geometry),  ALT = W^T [K][N] (backward-data).
 * bwd_data: dx[M][K] = dy[M][N] . W   (dy already multiplied by the activation derivative: evt_dact_mul)
 * bwd_weight: dw (fp32, REG geometry) += dy^T x ; dbias[N] (fp32, may be NULL) += column sums of dy. */
typedef struct evt_gemm_params {
  int32_t dtype;   /* EVT_DT_* */
  int32_t M, N, K;
  int32_t relu;    /* forward epilogue: max(0, .) */
} evt_gemm_params;
int evt_gemm_bf16_layout(const evt_gemm_params* g, evt_wlayout* out);
int evt_gemm_bf16_fwd(const evt_gemm_params* g, const void* x, const void* w_reg, const void* w_alt, const float* bias,
                      void* y, void* stream);
int evt_gemm_bf16_bwd_data(const evt_gemm_params* g, const void* dy, const void* w_reg, const void* w_alt, void* dx,
                           void* stream);
int evt_gemm_bf16_bwd_weight(const evt_gemm_params* g, const void* x, const void* dy, float* dw, float* dbias,
                             void* stream);

/* The same GEMMs with fused epilogues, on the 256 x 256 x 64 kernel of csrc/gemm256.hip (bf16, N and K multiples of 256 /
 * 64 on the output / reduction side, M >= 2048: the shapes of the s1 blocks at training batch sizes).  What the s1 block
 * (transformer.py:311-334) otherwise runs as separate element-wise launches rides in the GEMM's store:
 *   forward       y  = dropout(act(x . W^T + bias)) [+ add]     mask = counter hash of (*seed_dev, site, row * N + col),
 *                                                                the one evt_relu_dropout_fwd draws
 *   backward-data dx = (dy . W) * (gate > 0 ? gate_pos : 0) [+ add]
 *                 gate = the saved dropout(relu(.)) output of the layer below (its sign pattern IS the relu + dropout
 *                 derivative, gate_pos = 1 / (1 - p)); add = the residual branch's gradient.
 * evt_gemm_bf16_fused_supported says whether a shape is covered (callers fall back to the plain entry points plus the
 * element-wise launches); the _ex entry points return EVT_ENOTSUP otherwise.  epi may be NULL (plain GEMM). */
typedef struct evt_gemm_epilogue {
  float dropout_p;          /* 0 = off */
  uint32_t site;
  const uint32_t* seed_dev; /* device counter of the dropout stream (may be NULL = 0) */
  const void* gate;         /* [M][out columns] in the GEMM's dtype, or NULL */
  float gate_pos;
  uint32_t pad_;
  const void* add;          /* [M][out columns] in the GEMM's dtype, or NULL; added last */
} evt_gemm_epilogue;
int32_t evt_gemm_bf16_fused_supported(const evt_gemm_params* g, int32_t backward_data);
int evt_gemm_bf16_fwd_ex(const evt_gemm_params* g, const void* x, const void* w_reg, const void* w_alt, const float* bias,
                         const evt_gemm_epilogue* epi, void* y, void* stream);
int evt_gemm_bf16_bwd_data_ex(const evt_gemm_params* g, const void* dy, const void* w_reg, const void* w_alt,
                              const evt_gemm_epilogue* epi, void* dx, void* stream);

/* Flash attention with the ANALYTIC prefix-LM + key-padding mask of
 * src/easevoice/soundstorm/auto_reg/models/t2s_model.py:456-479 (no [B*H,L,L] mask tensor):
 *   key j visible from query i  <=>  j is not padding  AND  ( j < x_len  if i < x_len  else  j <= i )
 * where padding keys are x-part columns j >= x_lens[b] and y-part columns j - x_len >= y_lens[b].
 * q,k,v,o: [B][L][H][D] (the packed in_proj output viewed per head), D = 32 or 64, bf16 or fp32 storage;
 * softmax scale = 1/sqrt(D); lse: fp32 [B][H][L] (log-sum-exp, saved for backward).
 * Replaces F.scaled_dot_product_attention at patched_mha_with_cache.py:452-454. */
typedef struct evt_attn_params {
  int32_t dtype, B, L, H, D;
  int32_t x_len;             /* padded text length (prefix width) */
  int64_t q_stride_b, q_stride_l, q_stride_h; /* element strides (q, k, v share them) */
  int64_t o_stride_b, o_stride_l, o_stride_h;
  float dropout_p;           /* attention dropout on the normalised probabilities (SDPA dropout_p); 0 = off */
  uint32_t seed;             /* mask = hash(seed, b*H+h, query, key): identical in forward and backward */
} evt_attn_params;
int evt_attn_prefixlm_fwd(const evt_attn_params* p, const void* q, const void* k, const void* v,
                          const int32_t* x_lens, const int32_t* y_lens, void* o, float* lse, void* stream);
int evt_attn_prefixlm_bwd(const evt_attn_params* p, const void* q, const void* k, const void* v, const void* o,
                          const void* d_o, const float* lse, const int32_t* x_lens, const int32_t* y_lens,
                          void* dq, void* dk, void* dv, float* delta_ws, void* stream);

/* y = LayerNorm(x + r) * gamma + beta over the last dim C (post-LN block, transformer.py:311-315);
 * r may be NULL.  mean/rstd fp32 [rows] are saved for backward. */
int evt_add_layernorm_fwd(int32_t dtype, const void* x, const void* r, const float* gamma, const float* beta,
                          void* y, float* mean, float* rstd, int64_t rows, int32_t C, float eps, void* stream);
/* dxr = d/d(x+r); dgamma/dbeta fp32 [C] are accumulated (+=) */
int evt_add_layernorm_bwd(int32_t dtype, const void* x, const void* r, const float* gamma, const void* dy,
                          const float* mean, const float* rstd, void* dxr, float* dgamma, float* dbeta,
                          int64_t rows, int32_t C, void* stream);

/* ---------------------------------------------------------------------------------------
 * s2 transformer encoder glue (enc_p), src/easevoice/module/attentions.py:60-75.
 * ------------------------------------------------------------------------------------- */
/* *counter += inc, a 1-thread launch.  Device-side step / RNG counters: nothing about them is a host argument, so the
 * launches that read them can be replayed from a captured HIP graph. */
int evt_counter_inc(uint32_t* counter, uint32_t inc, void* stream);

/* out = LayerNorm(x + dropout(y)) * gamma + beta, rows (b, t) with t >= lens[b] written as zeros (lens may be NULL).
 * x, y, out [rows][C] in `dtype`; gamma/beta fp32 [C]; mean/rstd fp32 [rows] saved for the backward.
 * dropout keep(element) = hash(*seed_dev, site, element index) >= p * 2^32, kept values scaled by 1/(1-p); the backward
 * regenerates the mask from the same (seed, site).  rows_per_seq = T (row = b*T + t). */
int evt_res_dropout_ln_fwd(int32_t dtype, const void* x, const void* y, const float* gamma, const float* beta,
                           const int32_t* lens, int32_t rows_per_seq, float p, const uint32_t* seed_dev, uint32_t site,
                           void* out, float* mean, float* rstd, int64_t rows, int32_t C, float eps, void* stream);
/* dx = d(loss)/dx, dy = d(loss)/dy (= dx * dropout multiplier; may be NULL when p == 0: then dy == dx);
 * dgamma/dbeta fp32 [C] are accumulated (+=). */
int evt_res_dropout_ln_bwd(int32_t dtype, const void* x, const void* y, const float* gamma, const void* dout,
                           const float* mean, const float* rstd, const int32_t* lens, int32_t rows_per_seq, float p,
                           const uint32_t* seed_dev, uint32_t site, void* dx, void* dy, float* dgamma, float* dbeta,
                           int64_t rows, int32_t C, void* stream);

/* y = dropout(relu(x)) / dx = dy * dropout multiplier * (x > 0): the FFN inner activation of the s1 transformer blocks
 * (src/easevoice/soundstorm/auto_reg/modules/transformer.py:330-334), one pass each way; mask from the counter hash
 * (seed_dev, site, element index) as in evt_res_dropout_ln_*.  n % 8 == 0 (bf16) / % 4 (fp32), 16-byte aligned.
 * With lens != NULL the tensor is [.., rows_per_seq, C] and rows t >= lens[b] are zeroed (the `* x_mask` of the s2
 * encoder FFN, attentions.py:408-416); lens == NULL: no mask. */
int evt_relu_dropout_fwd(int32_t dtype, const void* x, float p, const uint32_t* seed_dev, uint32_t site,
                         const int32_t* lens, int32_t rows_per_seq, int32_t C, void* y, int64_t n, void* stream);
int evt_relu_dropout_bwd(int32_t dtype, const void* x, const void* dy, float p, const uint32_t* seed_dev, uint32_t site,
                         const int32_t* lens, int32_t rows_per_seq, int32_t C, void* dx, int64_t n, void* stream);

/* WN layer glue (src/easevoice/module/modules.py:199-211): rs = res_skip_layer(acts), [rows][2H] (H when last):
 *   last == 0:  x_out = (x + rs[:, :H]) * row_mask ;  acc_out = acc + rs[:, H:]     (acc may be NULL = zeros)
 *   last == 1:  acc_out = (acc + rs) * row_mask
 * backward: drs[:, :H] = dx = dx_out * row_mask, drs[:, H:] = dacc_out (last: drs = dacc_out * row_mask); d(acc) is
 * dacc_out itself and d(x) is dx.  dx_out / dacc_out may be NULL (= zeros). */
int evt_wn_residual_fwd(int32_t dtype, const void* x, const void* rs, const void* acc, const int32_t* lens,
                        int32_t rows_per_seq, void* x_out, void* acc_out, int64_t rows, int32_t H, int32_t last,
                        void* stream);
/* Element-wise chains of the style encoder (MelStyleEncoder, src/easevoice/module/modules.py:685-763), dropout masks from the
 * device counter + `site` as in evt_relu_dropout_*:
 *   Mish + Dropout (modules.py:521-545 LinearNorm / Mish / Dropout of `spectral`):  y = drop(x * tanh(softplus(x)))
 *   Conv1dGLU tail (modules.py:548-566):  y = res + drop(h[:, :C] * sigmoid(h[:, C:])),  h [rows][2C], res / y [rows][C]
 * backward: dx = dy * mask/(1-p) * mish'(x);  dh from dy (the residual's gradient is dy itself).
 * dtype: x / h and their gradients; wide_dtype: y / res / dy -- the same, or EVT_DT_F32 next to bf16 operands (the
 * reference's autocast keeps Mish outputs and the GLU residual stream in fp32 around its half-precision projections). */
int evt_mish_dropout_fwd(int32_t dtype, int32_t wide_dtype, const void* x, float p, const uint32_t* seed_dev, uint32_t site,
                         void* y, int64_t n, void* stream);
int evt_mish_dropout_bwd(int32_t dtype, int32_t wide_dtype, const void* x, const void* dy, float p, const uint32_t* seed_dev,
                         uint32_t site, void* dx, int64_t n, void* stream);
int evt_glu_dropout_res_fwd(int32_t dtype, int32_t wide_dtype, const void* h, const void* res, float p,
                            const uint32_t* seed_dev, uint32_t site, void* y, int64_t rows, int32_t C, void* stream);
int evt_glu_dropout_res_bwd(int32_t dtype, int32_t wide_dtype, const void* h, const void* dy, float p,
                            const uint32_t* seed_dev, uint32_t site, void* dh, int64_t rows, int32_t C, void* stream);
/* The style encoder on a RAGGED batch of references (inference: p = 0, forward only).  The reference's module convolves over
 * a tensor that ends at the clip's end, so every consumer with a footprint over time has to see zeros behind a row's length.
 * x / h / res / y [nseq][L][.], lens device int32 [nseq]; frame t of row s is live iff t < lens[s].
 *   evt_mish_rows_fwd:    y[s][t][c] = mish(x[s][t][c])                            live,  0 otherwise;  x, y [nseq][L][C]
 *   evt_glu_res_rows_fwd: y[s][t][c] = res[s][t][c] + h[s][t][c] * sigmoid(h[s][t][C + c])  live,  0 otherwise;  h [nseq][L][2C]
 * A live element is bit for bit what evt_mish_dropout_fwd / evt_glu_dropout_res_fwd give at p = 0, a dead one an exact zero
 * whatever x / h / res hold there (they are not read): one launch where that entry and evt_mask_tail were two.  dtype /
 * wide_dtype as above.  EVT_EINVAL for a NULL pointer, a size <= 0 or a pair of dtypes that is not served.
 *   evt_mean_rows: out[s][c] = (sum_{t < n_s} x[s][t][c]) / (float)n_s, n_s = min(max(lens[s], 0), L); x [nseq][L][C] of dtype,
 *   out fp32 [nseq][C], zeros for n_s = 0.  fp32 throughout.  Summation order: EVT_MEAN_ROWS_CHUNK = 64 consecutive frames
 *   counted from the row's frame 0 form a chunk; inside chunk k the frames 64 k + v, 64 k + v + 4, ... (v = 0 .. 3) are added
 *   in ascending order into four partial sums starting from 0, combined as (p0 + p1) + (p2 + p3); the chunk sums are added in
 *   ascending k, starting from 0 (the scheme of evt_hubert_front_rows, without a workspace).  Nothing but n_s enters: row s is
 *   bit for bit what nseq = 1 gives with any L >= n_s.  EVT_EINVAL for a NULL pointer, nseq <= 0 or > 65535, L or C <= 0, a
 *   dtype the build does not serve. */
#define EVT_MEAN_ROWS_CHUNK 64
int evt_mish_rows_fwd(int32_t dtype, int32_t wide_dtype, const void* x, const int32_t* lens, int32_t nseq, int32_t L,
                      int32_t C, void* y, void* stream);
int evt_glu_res_rows_fwd(int32_t dtype, int32_t wide_dtype, const void* h, const void* res, const int32_t* lens,
                         int32_t nseq, int32_t L, int32_t C, void* y, void* stream);
int evt_mean_rows(int32_t dtype, const void* x, const int32_t* lens, int32_t nseq, int32_t L, int32_t C, float* out,
                  void* stream);
/* Tail of the posterior encoder (src/easevoice/module/models.py:352-358): with stats [rows][2C] the projection's output,
 *   m = stats[:, :C] * mask, logs = stats[:, C:] * mask, z = (m + eps * exp(logs)) * mask     (fp32 [rows][C] each)
 * and its backward: dstats from dz / dm / dlogs (each may be NULL), eps and the saved logs. */
int evt_reparam_fwd(int32_t dtype, const void* stats, const float* eps, const int32_t* lens, int32_t rows_per_seq,
                    int64_t rows, int32_t C, float* z, float* m, float* logs, void* stream);
int evt_reparam_bwd(int32_t dtype, const float* dz, const float* dm, const float* dlogs, const float* eps, const float* logs,
                    const int32_t* lens, int32_t rows_per_seq, int64_t rows, int32_t C, void* dstats, void* stream);
/* Mean-only residual coupling + Flip of the s2 flow (src/easevoice/module/modules.py:404-458 forward with logs == 0 (mean_only),
 * models.py:273-315: flows = [coupling, Flip] x 4), everything after the layer's `post` projection in one launch:
 *   y[row][c] = v[row][2h-1-c],  v = [ x[:, :h] , (x[:, h:] + stats) * row_mask ];  x0n = y[:, :h] in `dtype` (the next
 *   layer's projection input) or NULL.  x, y fp32 [rows][2h]; stats [rows][h] in `dtype`; the row mask from lens as above. */
int evt_coupling_flip_fwd(int32_t dtype, const float* x, const void* stats, const int32_t* lens, int32_t rows_per_seq,
                          int64_t rows, int32_t h, float* y, void* x0n, void* stream);
/* dy [rows][2h] fp32 (+ dx0n [rows][h] in `dtype`, the gradient that arrived at x0n; may be NULL) ->
 * dx [rows][2h] fp32, dstats [rows][h] in `dtype` */
int evt_coupling_flip_bwd(int32_t dtype, const float* dy, const void* dx0n, const int32_t* lens, int32_t rows_per_seq,
                          int64_t rows, int32_t h, float* dx, void* dstats, void* stream);
int evt_wn_residual_bwd(int32_t dtype, const void* dx_out, const void* dacc_out, const int32_t* lens,
                        int32_t rows_per_seq, void* dx, void* drs, int64_t rows, int32_t H, int32_t last, void* stream);

/* Multi-head attention core of the s2 encoders: the windowed relative-position SELF-attention of enc_p
 * (attentions.py:214-292, window_size = w), the window-less CROSS-attention of MRTE (mrte_model.py:25-61 -> the same
 * MultiHeadAttention.attention with window_size = None, queries = ssl frames, keys / values = phonemes) and the style
 * encoder's ScaledDotProductAttention (modules.py:605-682, scale = 1/sqrt(d_model)):
 *   scores[i][j] = scale * (q_i . k_j + [window >= 0 and |j-i| <= w] q_i . Ek[j-i+w]);  keys j >= lens_k[b] excluded
 *   p = dropout(softmax_j(scores));   out_i = sum_j p[i][j] (v_j + [window >= 0 and |j-i| <= w] Ev[j-i+w])
 * q: rows [B][Tq][ldq], k, v: rows [B][Tk][ldk], head h in columns [h*D, (h+1)*D) (slices of one packed projection are
 * fine); out [B][Tq][ldo] likewise, all in `dtype` (bf16: MFMA flash kernels, D % 32 == 0; fp32: the 1e-3 parity path,
 * D % 4 == 0; D <= 128).  emb_k / emb_v fp32 [n_heads_rel][2w+1][D] (NULL when window < 0); lse fp32 [B*H][Tq] is saved
 * for the backward.  lens_q / lens_k int32 [B] or NULL (= all rows live).  Query rows i >= lens_q[b] are written as
 * zeros.  Dropout mask = hash(*seed_dev, site, b, h, i, j), regenerated by the backward. */
typedef struct evt_mha_params {
  int32_t dtype;           /* EVT_DT_* of q, k, v, out and their gradients */
  int32_t B, H, D;
  int32_t Tq, Tk;          /* query rows / key rows per item */
  int32_t window;          /* w >= 0: relative positions (needs Tq == Tk, 2w+1 <= 16); < 0: none */
  int32_t n_heads_rel;     /* 1 (heads share the embeddings) or H */
  int64_t ldq, ldk, ldo;   /* row strides in elements; 16-byte multiples */
  float scale;             /* logit scale: 1/sqrt(D) (attentions.py:257), 1/sqrt(d_model) (modules.py:618) */
  float dropout_p;
  uint32_t site;
  uint32_t pad_;
  const uint32_t* seed_dev;
} evt_mha_params;
int evt_mha_fwd(const evt_mha_params* p, const void* q, const void* k, const void* v, const float* emb_k,
                const float* emb_v, const int32_t* lens_q, const int32_t* lens_k, void* out, float* lse, void* stream);
/* dq (stride ldq), dk, dv (stride ldk) in `dtype`; demb_k / demb_v fp32, accumulated (+=), NULL when window < 0;
 * delta_ws fp32 [B*H][Tq] scratch. */
int evt_mha_bwd(const evt_mha_params* p, const void* q, const void* k, const void* v, const void* o, const void* d_o,
                const float* lse, const float* emb_k, const float* emb_v, const int32_t* lens_q, const int32_t* lens_k,
                void* dq, void* dk, void* dv, float* demb_k, float* demb_v, float* delta_ws, void* stream);

/* Cross-entropy, reduction="sum" (t2s_model.py:486-489): logits [rows][V] (any dtype), targets int64.
 * loss[0] += sum_r (lse_r - logit[r][t_r]); dlogits = (softmax - onehot) * dloss[0]; top-k hit counts for
 * the accuracy metric are written to hits[0] (+=, rows with target == ignore_index skipped, count in hits[1]). */
int evt_ce_sum_fwd_bwd(int32_t dtype, const void* logits, const int64_t* targets, void* dlogits, float* loss,
                       int32_t* hits, int64_t rows, int32_t V, int32_t topk, int64_t ignore_index, float dloss,
                       void* stream);
/* Per-row form for the DPO branch (t2s_model.py:420-427, models/utils.py:176-183): row_loss[r] = lse_r - logit[r][t_r]
 * (= -log p(target), written, not accumulated), dlogits = softmax - onehot (unscaled; the caller applies the per-row
 * upstream weight), hits as above.  The summed target log-probability of a sequence is -sum of its rows. */
int evt_ce_rows_fwd_bwd(int32_t dtype, const void* logits, const int64_t* targets, void* dlogits, float* row_loss,
                        int32_t* hits, int64_t rows, int32_t V, int32_t topk, int64_t ignore_index, void* stream);
/* The same two entry points for logits / dlogits with a row stride ld >= V (the GEMM above writes the 1025-entry
 * vocabulary into rows of 1152): columns [V, ld) of the logits are ignored and written as zeros in dlogits. */
int evt_ce_sum_fwd_bwd_ld(int32_t dtype, const void* logits, const int64_t* targets, void* dlogits, float* loss,
                          int32_t* hits, int64_t rows, int32_t V, int64_t ld, int32_t topk, int64_t ignore_index,
                          float dloss, void* stream);
int evt_ce_rows_fwd_bwd_ld(int32_t dtype, const void* logits, const int64_t* targets, void* dlogits, float* row_loss,
                           int32_t* hits, int64_t rows, int32_t V, int64_t ld, int32_t topk, int64_t ignore_index,
                           void* stream);

/* ---------------------------------------------------------------------------------------
 * s1 KV-cache decoding step (Text2SemanticDecoder.infer_panel_naive, t2s_model.py:762-863).
 * Every per-step quantity is device state, so the launches of a step take the same arguments for every token and can be
 * captured into a HIP graph.  ctr is a device int32[8]:
 * ------------------------------------------------------------------------------------- */
#define EVT_DEC_POS 0    /* key/value positions already in the cache */
#define EVT_DEC_IDX 1    /* decode step index (`idx` of t2s_model.py:822) */
#define EVT_DEC_YCOUNT 2 /* tokens in the y buffer (prompt + generated) */
#define EVT_DEC_YLEN 3   /* prompt length: the new token's position is YLEN + IDX (t2s_model.py:861) */
#define EVT_DEC_SEED 4   /* per-call sampling seed, xor-ed with evt_sample_params.seed */
/* y[b][n] = act(bias[n] + sum_k W[n][k] * x[b][k]); W [N][K] row-major in `wdtype`, vectors fp32, B <= 4 (sessions of up
 * to four rows; evt_dec_gemm_rows below serves up to 128), K % 512 == 0.
 * r == NULL: x = a.  r != NULL: x = LayerNorm(a + r) * ln_g + ln_b (the post-LN residual of T2SBlock.decode_next_token,
 * t2s_model.py:208-221, recomputed per workgroup); x_out (may be NULL) receives it for the next residual and must not
 * alias a or r.  relu != 0 applies max(0, .) (T2SMLP.forward, t2s_model.py:74-77). */
int evt_dec_gemv(int32_t wdtype, const void* W, const float* bias, const float* a, const float* r, const float* ln_g,
                 const float* ln_b, float ln_eps, float* x_out, float* y, int32_t B, int32_t N, int32_t K, int32_t relu,
                 void* stream);
/* evt_dec_gemv for 1 <= B <= 128 rows (the wide decode sessions of 5..32 texts, t2s_model.py:563-730, and stream sessions
 * of up to 128 slots): same arguments and numerics (x fp32, 16-bit weights widened exactly, fp32 products and sums; only
 * the order of the sum differs), but every weight byte is read from HBM once per launch for all rows (fp32-input MFMA
 * over 16-row tiles of W).  More than 32 rows run as row groups of 32, one more grid dimension: every output row has the
 * bits a launch of that row's group alone (rows 32g .. 32g+31 of a, r) gives, and a weight tile is read once per
 * group (the re-reads are meant to hit L2 / the Infinity Cache; not measured).  B > 128: EVT_ENOTSUP.  K % 512 == 0, K <= 2048; W, a, r, ln_g, ln_b and x_out 16-byte aligned.
 * Deterministic: no atomics. */
int evt_dec_gemm_rows(int32_t wdtype, const void* W, const float* bias, const float* a, const float* r,
                      const float* ln_g, const float* ln_b, float ln_eps, float* x_out, float* y, int32_t B, int32_t N,
                      int32_t K, int32_t relu, void* stream);
/* qkv fp32 [B][3*H*D] of the new token: its key/value are stored at cache position ctr[POS] (kcache/vcache
 * [B][Lmax][H*D] in `cdtype`) and out[b][h*D+d] = softmax(q.K^T/sqrt(D)).V over positions 0..ctr[POS]
 * (t2s_model.py:187-204 without the torch.cat growth).  D == 32.
 * x_lens (may be NULL): int32 [B]; cache positions x_lens[b] <= j < x_len are the padding of a shorter text in a batch
 * (the padding mask of infer_panel_batch_infer, t2s_model.py:620-650) and are not attended. */
int evt_dec_attn(int32_t cdtype, const float* qkv, void* kcache, void* vcache, const int32_t* ctr, float* out, int32_t B,
                 int32_t H, int32_t D, int32_t Lmax, const int32_t* x_lens, int32_t x_len, void* stream);
/* evt_dec_gemv (the packed in-projection) and evt_dec_attn in one launch: workgroup (b, h) computes only its head's
 * 3*D rows of Wqkv [3*H*D][H*D] (+ bqkv) from x = a or LayerNorm(a + r) (workgroups h == 0 store it to x_out), then
 * appends and attends as evt_dec_attn does.  The weights and the cache share `dtype`.  H*D == 512, D == 32. */
int evt_dec_qkv_attn(int32_t dtype, const void* Wqkv, const float* bqkv, const float* a, const float* r,
                     const float* ln_g, const float* ln_b, float ln_eps, float* x_out, void* kcache, void* vcache,
                     const int32_t* ctr, float* out, int32_t B, int32_t H, int32_t D, int32_t Lmax, const int32_t* x_lens,
                     int32_t x_len, void* stream);
/* sample() of models/utils.py:125-171 for one step: the EOS column is dropped while ctr[IDX] < no_eos_steps
 * (t2s_model.py:833-834); repetition penalty over y[b][0..ctr[YCOUNT]); nucleus cut (top_p < 1) on the un-tempered
 * logits; division by max(temperature, 1e-5); top-k pivot (top_k <= 0: off; ties kept); softmax;
 * token = argmax(probs / q) with q = noise[ctr[IDX]][v] (noise fp32 [steps][V]) or, when noise == NULL, exponential
 * noise from a counter hash of (seed ^ ctr[SEED], step, b, v).  The token is written to y[b][ctr[YCOUNT]] (y int64 [B][ymax]);
 * stop_idx[b] (int32, initialised to -1 by the caller) receives the first step at which argmax of the penalised logits
 * or the token equals eos (t2s_model.py:846).  probs_out (may be NULL) fp32 [B][V]. */
typedef struct evt_sample_params {
  int32_t V, eos, top_k, no_eos_steps, ymax;
  float top_p, temperature, repetition_penalty;
  uint32_t seed;
  int32_t noise_rows;   /* 1: noise [steps][V] shared by the batch rows; B: noise [steps][B][V] */
} evt_sample_params;
int evt_dec_sample(const evt_sample_params* p, const float* logits, int64_t* y, const int32_t* ctr, const float* noise,
                   int32_t* stop_idx, float* probs_out, int32_t B, void* stream);
/* evt_dec_sample with the built-in noise of row b keyed by the device table row_seed int32 [B][2] = (seed, lane) where
 * evt_dec_sample uses (ctr[SEED], b): a wide session of up to 32 rows draws, row for row, the noise that groups of four
 * rows seeded (seed + 4*g) draw in evt_dec_sample. */
int evt_dec_sample_rows(const evt_sample_params* p, const float* logits, int64_t* y, const int32_t* ctr,
                        const float* noise, int32_t* stop_idx, float* probs_out, const int32_t* row_seed, int32_t B,
                        void* stream);
/* evt_dec_sample + evt_dec_embed + evt_dec_advance(dpos) for ONE sequence in a single launch */
int evt_dec_sample_embed(const evt_sample_params* p, const float* logits, int64_t* y, int32_t* ctr, const float* noise,
                         int32_t* stop_idx, const float* emb, const float* pe, const float* alpha, float x_scale, float* x,
                         int32_t E, int32_t npos, int32_t dpos, void* stream);
/* x[b] = emb[y[b][ctr[YCOUNT]]] * x_scale + alpha[0] * pe[ctr[YLEN] + ctr[IDX]]  (t2s_model.py:860-861); emb fp32
 * [V][E], pe fp32 [npos][E]. */
int evt_dec_embed(const float* emb, const float* pe, const float* alpha, float x_scale, const int64_t* y,
                  const int32_t* ctr, float* x, int32_t B, int32_t E, int32_t ymax, int32_t npos, void* stream);
/* end of a step: ctr[IDX] += 1, ctr[YCOUNT] += 1, ctr[POS] += dpos (1 after a decode step, 0 after the prompt pass) */
int evt_dec_advance(int32_t* ctr, int32_t dpos, void* stream);

/* Per-row decode state of a continuously batched session (csrc/s1_decode_stream.hip): rstate is a device int32
 * [B][EVT_ROW_WORDS].  With the counters per row, rows of one session may have different prompt lengths, start at
 * different times and stop on their own, and a finished row's slot can be refilled between two steps. */
#define EVT_ROW_WORDS 8
#define EVT_ROW_POS 0      /* key/value positions of this row already in its cache slab */
#define EVT_ROW_IDX 1      /* the row's own decode step index */
#define EVT_ROW_YCOUNT 2   /* tokens in the row's y buffer (prompt + generated) */
#define EVT_ROW_YLEN 3     /* the row's prompt length */
#define EVT_ROW_LIMIT 4    /* the row stops after the step IDX == LIMIT - 1 at the latest */
#define EVT_ROW_STATUS 5   /* EVT_ROW_IDLE | RUNNING | STOP_EOS | STOP_LIMIT */
#define EVT_ROW_NOISE 6    /* column of an injected noise table [steps][noise_rows][V] this row reads */
#define EVT_ROW_NFORCE 7   /* forced steps: while IDX < NFORCE, evt_dec_sample_embed_rows_f takes the token from y */
#define EVT_ROW_SPARE EVT_ROW_NFORCE   /* the word's name while it was unused; the other entry points ignore it */
#define EVT_ROW_IDLE 0
#define EVT_ROW_RUNNING 1
#define EVT_ROW_STOP_EOS 2
#define EVT_ROW_STOP_LIMIT 3
/* evt_dec_attn with the cache length of row b taken from rstate[b][POS]: appends the new key/value at that position of
 * the row's slab and attends over positions 0..POS except the padding x_lens[b] <= j < x_len.  A row whose status is not
 * RUNNING is skipped: nothing is appended and out[b] is left as it is.  Arithmetic and summation order are those of
 * evt_dec_attn, so a row equals a one-row evt_dec_attn call at its position bit for bit. */
int evt_dec_attn_rows(int32_t cdtype, const float* qkv, void* kcache, void* vcache, const int32_t* rstate, float* out,
                      int32_t B, int32_t H, int32_t D, int32_t Lmax, const int32_t* x_lens, int32_t x_len, void* stream);
/* One launch for the end of a step of all B rows: the sampling of evt_dec_sample_rows with IDX / YCOUNT / YLEN of the
 * row (no_eos_steps against the row's own IDX; built-in noise keyed by row_seed[b] and the row's IDX; an injected table
 * read at [IDX][rstate[b][NOISE]]), the append to y[b], x[b] = emb[token] * x_scale + alpha[0] * pe[YLEN + IDX], and
 * the row's counter update.  On EOS (arg-max of the penalised logits or the token), or when IDX + 1 reaches LIMIT, the
 * row's status becomes STOP_EOS / STOP_LIMIT and stop_idx[b] receives IDX; the counters then stay.  Otherwise
 * POS += dpos (1 in a decode step, 0 after the prompt pass), IDX += 1, YCOUNT += 1.  Rows that are not RUNNING are
 * skipped, and so are rows with row_mask[b] == 0 when row_mask (int32 [B], may be NULL) is given: step 0 of freshly
 * admitted rows.  probs_out may be NULL. */
int evt_dec_sample_embed_rows(const evt_sample_params* p, const float* logits, int64_t* y, int32_t* rstate,
                              const float* noise, int32_t* stop_idx, float* probs_out, const int32_t* row_seed,
                              const int32_t* row_mask, const float* emb, const float* pe, const float* alpha,
                              float x_scale, float* x, int32_t B, int32_t E, int32_t npos, int32_t dpos, void* stream);
/* evt_dec_sample_embed_rows with top_k, top_p, temperature and repetition_penalty of row b read from row_sample[b]
 * (device memory, [B]) instead of p; V, eos, no_eos_steps, ymax, seed and noise_rows stay in p.  A table whose entries
 * all equal p's values gives evt_dec_sample_embed_rows bit for bit.  The launcher cannot see the table: the caller keeps
 * repetition_penalty > 0 and every float finite (no table value can move a memory access, see the kernel). */
typedef struct evt_row_sample { int32_t top_k; float top_p, temperature, repetition_penalty; } evt_row_sample;  /* 16 bytes */
int evt_dec_sample_embed_rows_p(const evt_sample_params* p, const evt_row_sample* row_sample, const float* logits,
                                int64_t* y, int32_t* rstate, const float* noise, int32_t* stop_idx, float* probs_out,
                                const int32_t* row_seed, const int32_t* row_mask, const float* emb, const float* pe,
                                const float* alpha, float x_scale, float* x, int32_t B, int32_t E, int32_t npos,
                                int32_t dpos, void* stream);
/* evt_dec_sample_embed_rows_p that also writes, for every row it advances, two fp32 log-probabilities of the drawn
 * token to row_logp[b][YCOUNT] (row_logp: device [B][ymax][2]; YCOUNT as it is BEFORE the launch, the index at which
 * the token is appended to y[b]):
 *   [0]  log_softmax of the raw logits[b] over the columns of that step (V - 1 while IDX < no_eos_steps, else V) at
 *        the token: no repetition penalty, no nucleus / top-k cut, no temperature;
 *   [1]  the log of the probability the token was drawn from after all of those, x - max - log(sum) of the values the
 *        sampler's softmax is taken of (never -inf for a token that survived the cuts).
 * A token outside [0, V) (NaN probabilities) gives NaN in both.  Idle, stopped and masked-out rows write nothing.  y,
 * rstate, stop_idx, x and probs_out are those of evt_dec_sample_embed_rows_p bit for bit. */
int evt_dec_sample_embed_rows_lp(const evt_sample_params* p, const evt_row_sample* row_sample, const float* logits,
                                 int64_t* y, int32_t* rstate, const float* noise, int32_t* stop_idx, float* probs_out,
                                 const int32_t* row_seed, const int32_t* row_mask, const float* emb, const float* pe,
                                 const float* alpha, float x_scale, float* x, float* row_logp, int32_t B, int32_t E,
                                 int32_t npos, int32_t dpos, void* stream);
/* evt_dec_sample_embed_rows_lp in which row_logp may be NULL (then it is evt_dec_sample_embed_rows_p) and a row may have
 * FORCED steps.  With nforce = rstate[b][EVT_ROW_NFORCE], a step of row b with IDX < nforce takes its token from
 * y[b][YCOUNT], where the caller has written it, instead of the sampler's draw.  Everything after the token is as ever:
 * the append (which rewrites the value), x[b], the counters, the LIMIT test.  The row stops with STOP_EOS when the given
 * token is eos; the arg-max rule is NOT applied in a forced step (the given sequence decides where it ends) and both
 * rules apply again from step nforce on.  IDX counts through forced steps and keys the noise as ever, so the first
 * sampled step after k forced ones reads noise row k (built-in noise: hash of IDX = k): a row forced over a prefix of
 * what it once sampled continues exactly as it did.  row_logp of a forced step:
 *   [0]  log_softmax of the raw logits over the step's columns at the given token (-inf for eos at a step without it);
 *   [1]  the log of the probability the sampler would have drawn the token from after penalty, nucleus, top-k and
 *        temperature: -inf when the sampler had cut it.
 * A given token outside [0, V) is stored as 0x7fffffff, embeds row 0 and reports NaN; the caller validates what it
 * writes.  A row with nforce = 0 is, in every bit, a row of evt_dec_sample_embed_rows_lp / _p. */
int evt_dec_sample_embed_rows_f(const evt_sample_params* p, const evt_row_sample* row_sample, const float* logits,
                                int64_t* y, int32_t* rstate, const float* noise, int32_t* stop_idx, float* probs_out,
                                const int32_t* row_seed, const int32_t* row_mask, const float* emb, const float* pe,
                                const float* alpha, float x_scale, float* x, float* row_logp, int32_t B, int32_t E,
                                int32_t npos, int32_t dpos, void* stream);

/* ScaledAdam (src/easevoice/soundstorm/auto_reg/modules/optim.py:206-251,300-390,448-622) over a flat fp32 arena.
 * The reference stacks same-shaped tensors only to batch its torch ops; the arithmetic is per tensor, which is what
 * these two launches implement for ALL tensors at once:
 *   evt_scaled_adam_stats : stats[t] = (sum p*g, sum p*p, sum g*g) per tensor t  (+=, caller zeroes stats)
 *   evt_scaled_adam_apply : delta = beta1*delta + p*coef[t][0] + g/(sqrt(v_hat)+eps)*coef[t][1] ; p += delta
 *                           (coef[t][2] != 0 selects the numel==1 "scalar" branch, optim.py:600-622).  As in the
 *                           reference, gradient clipping only enters through coef[t][0] (the size update).
 * The per-tensor scalars between the two launches (size update, clipping scale) are a few vector ops on [ntensor]
 * device arrays done by the host layer.  chunks: DEVICE table, one workgroup per chunk (a slice of one tensor). */
typedef struct evt_sa_chunk { int64_t begin, end; int32_t tensor; int32_t pad_; } evt_sa_chunk;
typedef struct evt_scaled_adam_hp {
  float lr, beta1, beta2, eps, scalar_lr_scale, scalar_max;
  int32_t step, pad_;
} evt_scaled_adam_hp;
int evt_scaled_adam_stats(const float* param, const float* grad, const evt_sa_chunk* chunks, int32_t nchunks,
                          float* stats, void* stream);
int evt_scaled_adam_apply(float* param, const float* grad, float* delta, float* exp_avg_sq, const evt_sa_chunk* chunks,
                          int32_t nchunks, const float* coef, const evt_scaled_adam_hp* hp, void* stream);

/* ---------------------------------------------------------------------------------------
 * Feature extractors behind the training set (src/normalization/normalize.py:88-106 `_get_bert_feature`,
 * :132-180 `_name2go` of the reference: transformers' BertForMaskedLM / HubertModel on the CPU).  Their transformer
 * layers run on the entry points above (1x1 convolutions = the Linear layers, evt_mha_fwd, evt_res_dropout_ln_fwd);
 * these two are what they need besides.  Forward only (inference).
 *   evt_gelu_rows_fwd: out[b][t][:] = gelu(x[b][t][:] + bias) for t < t_out <= t_in, erf form (transformers' "gelu");
 *     x [nseq][t_in][C], out [nseq][t_out][C], bias fp32 [C] or NULL.  t_out = t_in - 1 is the trim of HuBERT's positional
 *     convolution (HubertSamePadLayer drops the last frame of an even kernel).
 *   evt_channel_norm_gelu_fwd: per (sequence, channel) normalisation over the T frames, affine, then GELU if apply_gelu:
 *     GroupNorm(num_groups = C) + GELU of HuBERT's first feature-extractor layer.  x, out [nseq][T][C]; biased variance. */
int evt_gelu_rows_fwd(int32_t dtype, const void* x, const float* bias, void* out, int64_t nseq, int32_t t_in, int32_t t_out,
                      int32_t C, void* stream);
int evt_channel_norm_gelu_fwd(int32_t dtype, const void* x, const float* gamma, const float* beta, float eps, void* out,
                              int32_t nseq, int32_t T, int32_t C, int32_t apply_gelu, void* stream);

/* HuBERT's first feature-extractor layer (Conv1d(1, 512, k = 10, stride 5, no bias) -> GroupNorm(512, 512) -> GELU) for a
 * RAGGED batch of clips, without materialising the convolution: the clip front end of CNHubert.batch.
 *   wav [nseq][N] fp32; lens device int32 [nseq] in samples, row s has n_s = min(max(lens[s], 0), N) live samples and wav is
 *   never read at or behind them; w fp32 [512][10]; gamma, beta fp32 [512].
 *   out [nseq][T1][512] of dtype, T1 = (N - 10) / 5 + 1.  Row s has T_s = (n_s - 10) / 5 + 1 frames (0 when n_s < 10):
 *     c[t][ch] = sum_{j < 10} w[ch][j] * wav[s][5 t + j]     (fp32 fma chain, j ascending from 0)
 *     mean[ch] = sum_t c / T_s;  var[ch] = sum_t (c - mean)^2 / T_s  (biased; two passes, never E[x^2] - E[x]^2)
 *     out[s][t][ch] = gelu_erf((c - mean) * rsqrt(var + eps) * gamma[ch] + beta[ch])   t < T_s, rounded once
 *     out[s][t][:]  = 0                                                                T_s <= t < T1
 *   Every element of out is written.
 * Summation order: a block owns EVT_HUBERT_FRONT_CHUNK consecutive frames of one row counted from the row's frame 0; inside
 * a chunk, frames t = v, v + 4, ... (v = 0 .. 3) are added in ascending order into four partial sums, combined as
 * (p0 + p1) + (p2 + p3); the per-chunk sums go to the workspace and are added in ascending chunk order.  Neither nseq nor N
 * enters: row s is bit for bit what the entry gives for that row alone (nseq = 1) with any N >= n_s.
 * Five launches on `stream` (chunk sums, mean, chunk sums of squared deviations, rstd, normalise + GELU + store; the second
 * and third pass recompute the convolution from the staged samples), no host synchronisation: legal in a captured graph.
 * ws: fp32 workspace of at least evt_hubert_front_ws_floats(nseq, N) = nseq * 512 * (ceil(T1 / CHUNK) + 2) floats, 16-byte
 * aligned, contents undefined afterwards.  EVT_EINVAL for a NULL pointer, nseq <= 0 or > 65535, N < 10, eps < 0 or NaN,
 * ws_floats too small, out or ws not 16-byte aligned; EVT_ENOTSUP for a dtype the build does not serve.  The query returns
 * 0 for arguments the entry refuses. */
#define EVT_HUBERT_FRONT_CHUNK 64
int64_t evt_hubert_front_ws_floats(int32_t nseq, int32_t N);
int evt_hubert_front_rows(int32_t dtype, const float* wav, const int32_t* lens, int32_t nseq, int32_t N, const float* w,
                          const float* gamma, const float* beta, float eps, void* out, float* ws, int64_t ws_floats,
                          void* stream);

/* The clip rescaling of the reference's `ssl` step (src/normalization/normalize.py:148-153, restated for one clip by
 * feature_extractor/normalize.py::rescale_clip) for a ragged batch of 32 kHz clips.  x [nseq][N] fp32, lens device int32
 * [nseq], n_s = min(max(lens[s], 0), N), x never read at or behind n_s.  Two launches, no host synchronisation:
 *   peak[s] = max_{i < n_s} |x[s][i]|  (fp32 [nseq], an OUTPUT; NaN if the row holds a NaN, 0 for an empty row)
 *   f[s][i] = fadd(fmul(fdiv(x, peak), c1b), fmul(c2b, x))         fp32 [nseq][N]: the clip that is resampled for HuBERT
 *   q[s][i] = (int16) trunc(fadd(fmul(fdiv(x, peak), c1), fmul(c2, x)))  int16 [nseq][N]: the clip written to 5-wav32k
 *   f = 0, q = 0 for n_s <= i < N
 * every operation rounded to fp32 on its own (round to nearest even, no contraction into an fma), as numpy evaluates the
 * float32 expression; c1 = (float)(0.95 * 0.5 * 32768), c2 = (float)(0.5 * 32768), c1b = (float)(0.95 * 0.5 * 1145.14),
 * c2b = (float)(0.5 * 1145.14), the products taken in double.  For a clip whose peak is <= 1 the value under the cast is at
 * most 31 948.8 in magnitude and q equals numpy's astype(int16) bit for bit.  Outside the int16 range, where numpy's cast is
 * undefined, q SATURATES to [-32768, 32767], and a NaN (a NaN sample, or 0 / 0 in a silent clip) gives q = 0.
 * EVT_EINVAL for a NULL pointer, nseq <= 0 or > 65535, N <= 0. */
int evt_clip_rescale_rows(const float* x, const int32_t* lens, int32_t nseq, int32_t N, float* f, int16_t* q, float* peak,
                          void* stream);

/* The output end of Chinese-RoBERTa's phone-level features for a group of sentences: a transposing gather, one launch.
 *   h [B][T][C] of dtype, 16-byte aligned; src device int32 [total]: for every output column the flat token row b * T + t
 *   it copies, or -1 for a column of zeros (a value outside [-1, B * T) is taken as -1 on the device, never read);
 *   item_off device int32 [n_items + 1]: item i owns columns item_off[i] .. item_off[i + 1] - 1, n_i of them (0 is legal).
 *   out, packed, of out_dtype (fp32 or the build's 16-bit type, rounded to nearest even): item i is a contiguous [C][n_i]
 *   block at element C * item_off[i],
 *     out[C * item_off[i] + c * n_i + (p - item_off[i])] = h[src[p]][c], or 0.
 *   Every element of out[0, C * total) that belongs to an item is written once, nothing else is; token rows that no
 *   column names are never read.  item_off is expected ascending from 0 to total; every entry is clamped into
 *   [previous end, total] on the device, so a wrong one cannot send a store outside out.
 * A block owns 64 consecutive columns of one item (a tile never crosses an item) and 64 channels: 16-byte reads along c,
 * an LDS tile of 65-word rows (both sides at most 2-way conflicted), stores of 64 consecutive columns per wave.  Plain
 * vector stores, no atomics, no host synchronisation: legal in a captured graph.
 * EVT_EINVAL (nothing launched) for a NULL h / item_off (src / out when total > 0), B, T or n_items <= 0, n_items > 65535,
 * B * T >= 2^31, C outside 8 .. 4096 or not a multiple of 8, total < 0, h not 16-byte aligned; EVT_ENOTSUP for a dtype the
 * build does not serve.  total == 0 is EVT_OK without a launch. */
int evt_phone_expand_rows(int32_t dtype, const void* h, int32_t B, int32_t T, int32_t C, const int32_t* src,
                          const int32_t* item_off, int32_t n_items, int32_t total, int32_t out_dtype, void* out,
                          void* stream);

/* The input end: BERT's embedding sum and its LayerNorm for a right-padded group of sentences, one launch.
 *   ids int32 [B][T]; tt int32 [B][T] token types or NULL (all 0); lens device int32 [B], row b has
 *   min(max(lens[b], 0), T) live tokens; word fp32 [vocab][C], pos fp32 [max_pos][C], type fp32 [types][C], gamma, beta
 *   fp32 [C], all 16-byte aligned.
 *     v[c]         = (word[id][c] + pos[t][c]) + type[ty][c]          fp32; id, ty clamped into their tables on the device
 *     mean         = sum_c v / C;  var = sum_c (v - mean)^2 / C       two passes
 *     out[b][t][c] = (v - mean) / sqrt(var + eps) * gamma[c] + beta[c]   t <  lens[b], rounded once to dtype
 *     out[b][t][:] = 0                                                   t >= lens[b]  (ids there are not read)
 * One wave per token row; lane l adds channels 4 l + 256 i in ascending i, four at a time as (a + b) + (c + d), the wave sum
 * is the xor butterfly 32, 16, .., 1: the order depends on C alone, so a row is bit for bit the same for any B and any
 * T >= lens[b].  No host synchronisation.
 * EVT_EINVAL (nothing launched) for a NULL pointer other than tt, B, T, vocab or types <= 0, T > max_pos, B * T >= 2^31, C
 * outside 4 .. 8192 or not a multiple of 4, eps < 0 or NaN, a table or out not 16-byte aligned; EVT_ENOTSUP for a dtype the
 * build does not serve. */
int evt_bert_embed_ln_rows(int32_t dtype, const int32_t* ids, const int32_t* tt, const int32_t* lens, int32_t B, int32_t T,
                           const float* word, int32_t vocab, const float* pos, int32_t max_pos, const float* type,
                           int32_t types, const float* gamma, const float* beta, float eps, int32_t C, void* out,
                           void* stream);

/* The audio slicer (src/audiokit/slicer/slicer.py, AudioService.slicer of the reference) on a ragged batch of recordings.
 * The recordings lie in ONE packed fp32 buffer x of x_len elements: recording r is x[off[r] : off[r] + len[r]], off and
 * len device int64, 1 <= len[r] < 2^31.  Nothing outside a recording's (a span's) own elements is read; an entry that
 * does not lie inside [0, x_len) is skipped on the device (its outputs are not written).  No host synchronisation.
 *
 * evt_rms_frames_rows: get_rms (slicer.py:149-180).  Recording r has F_r = (len_r + 2 * (win / 2) - win) / hop + 1 frames
 * (integer divisions); frame f is
 *     rms[frame_off[r] + f] = fsqrt(fdiv(sum_k fmul(v_k, v_k), (float)win)),  v_k = x_r[f * hop - win / 2 + k], k < win,
 * samples outside [0, len_r) taken as 0.  frame_off device int64 [nrec + 1]: the prefix sum of F_r from 0 to total_frames
 * (the host's; rms has total_frames elements, nothing behind them is written).  The win additions are taken in the order
 * of NumPy's pairwise float32 summation of a contiguous run of n values:
 *     n < 8:    sequential;
 *     n <= 128: eight accumulators r[j] = a[j], r[j] += a[i + j] for i = 8, 16, .. < n - n % 8, then
 *               ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 leftovers one by one;
 *     n > 128:  n2 = n / 2, n2 -= n2 % 8, sum(a[:n2]) + sum(a[n2:]), recursively;
 * every operation rounded to fp32 on its own, division and square root correctly rounded: a frame equals the reference's
 * bit for bit, and it does not depend on the other recordings of the buffer.  One wave per frame.
 * EVT_EINVAL for a NULL pointer or x_len, nrec, win, hop, total_frames <= 0; EVT_ENOTSUP for win > 8192. */
int evt_rms_frames_rows(const float* x, int64_t x_len, const int64_t* off, const int64_t* len, int32_t nrec, int32_t win,
                        int32_t hop, float* rms, const int64_t* frame_off, int64_t total_frames, void* stream);

/* peak[s] = max_{i < n[s]} |x[src_off[s] + i]| for nspan spans of the buffer (src_off, n device int64): fp32 [nspan], a NaN
 * if the span holds one (as np.abs(x).max()), 0 for n[s] == 0.  max_n: an upper bound of the n[s] the host knows (it sizes
 * the grid; a larger span is still served).  A memset of peak and one launch.
 * EVT_EINVAL for a NULL pointer, x_len <= 0, nspan <= 0 or > 65535, max_n < 0. */
int evt_span_peak_rows(const float* x, int64_t x_len, const int64_t* src_off, const int64_t* n, int32_t nspan, int64_t max_n,
                       float* peak, void* stream);

/* The per-chunk arithmetic of AudioService.slicer (audio.py:172-178) for nspan chunks in one launch, in numpy's float32
 * steps (fdiv / fmul / fadd, each rounded on its own), i < n[s]:
 *     v = x[src_off[s] + i];  if (peak[s] > 1) v = fdiv(v, peak[s]);
 *     w = fadd(fmul(fdiv(v, peak[s]), c1), fmul(c2, v))
 *     out[dst_off[s] + i] = (int16) trunc(fmul(w, 32767.0f))
 * c1 = (float)(normalize_max * alpha_mix), the product in double; c2 = (float)(1 - alpha_mix).  peak[s] == 0 is an all-zero
 * chunk, where numpy casts a NaN (undefined): zeros are written for it.  out int16 of out_len elements; a chunk that does
 * not fit into it is skipped.  The cast saturates and maps NaN to 0, as evt_clip_rescale_rows does.
 * EVT_EINVAL for a NULL pointer, x_len or out_len <= 0, nspan <= 0 or > 65535, max_n < 0. */
int evt_slice_pack_rows(const float* x, int64_t x_len, const int64_t* src_off, const int64_t* n, const int64_t* dst_off,
                        const float* peak, float c1, float c2, int32_t nspan, int64_t max_n, int16_t* out, int64_t out_len,
                        void* stream);

/* Semantic codes of a ragged batch of CN-HuBERT hidden states (models.py:1015-1018: ssl_proj, a Conv1d D -> D with k = 2 and
 * stride 2, + the nearest code of the frozen codebook, n_q = 1) in one launch, fp32 throughout on the fp32-input MFMA.
 *   hs [B][Tmax][D] channels-last of dtype (fp32 or the build's 16-bit type, widened on load); frames device int32 [B];
 *   offsets device int64 [B + 1]: the exclusive prefix sum of frames[b] / 2 (integer division), offsets[B] = total;
 *   proj_image fp32 [2 D][D]: row tap * D + c, column o holds ssl_proj.weight[o][c][tap]; bias fp32 [D]; embed fp32 [K][D];
 *   ee fp32 [K] from evt_rvq_norms.
 * Row b gets frames[b] / 2 codes at codes[offsets[b] ..] (int64, `total` elements; an odd last frame is dropped):
 *     h_t = bias + sum_{tap, c} hs[b][2 t + tap][c] * proj_image[tap * D + c][.],   xx = sum_d h_t[d]^2,
 *     code = the smallest k among the maxima of -((xx - 2 h_t . embed[k]) + ee[k]), 0 when no k has one (an all-NaN frame):
 * evt_rvq_select's decision.  A block owns EVT_SEMANTIC_TILE code frames of one row counted from its frame 0; h, the dots
 * and the code vectors are never written to memory, and every sum has an order fixed by D and K alone, so a row's codes are
 * bit for bit those of nseq = 1 with any Tmax >= frames[b].  Nothing at or behind frame frames[b] of a row is read (the
 * device clamps frames[b] to 0 .. Tmax), nothing of a row with fewer than two frames; no code is written outside `total`.
 * frames_host (may be NULL): the host's copy of frames, checked here.
 * EVT_EINVAL (nothing launched) for a NULL pointer other than frames_host (codes when total > 0), B <= 0 or > 65535,
 * Tmax <= 0, K <= 0, total < 0, D not a multiple of 64 or above EVT_SEMANTIC_MAX_D (h must fit LDS), hs / proj_image / bias /
 * embed not 16-byte aligned, a dtype the build does not serve, a frames_host[b] outside 0 .. Tmax.  total == 0 is EVT_OK
 * without a launch. */
#define EVT_SEMANTIC_TILE 32
#define EVT_SEMANTIC_MAX_D 1152
int evt_semantic_codes_rows(int32_t dtype, const void* hs, const int32_t* frames, const int32_t* frames_host,
                            const int64_t* offsets, int32_t B, int32_t Tmax, int32_t D, int32_t K, const float* proj_image,
                            const float* bias, const float* embed, const float* ee, int64_t* codes, int64_t total,
                            void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EVT_H */

"""Bindings of the feature extractors' own launches (csrc/feat_ops.hip, csrc/pos_conv.hip, csrc/semantic.hip,
csrc/mha_rows.hip, csrc/gemm_rows.hip) and the LayerNorm entry point they share with the s1 blocks.  Inference only: nothing here records an
autograd graph."""
import ctypes as C

import torch

from . import lib as L
from . import trace as T


def gelu_rows(x, bias=None, t_out=None):
    """x [B, T, C] -> gelu(x + bias)[:, :t_out] (erf form), one launch; bias fp32 [C] or None"""
    if x.dim() != 3 or not x.is_contiguous():
        raise L.EvtError(f"gelu_rows: contiguous [B, T, C] expected, got {tuple(x.shape)}")
    B, T, Cc = x.shape
    t_out = T if t_out is None else int(t_out)
    out = torch.empty((B, t_out, Cc), dtype=x.dtype, device=x.device)
    L.check(L.lib().evt_gelu_rows_fwd(L.dt_of(x), L.ptr(x), L.ptr(bias), L.ptr(out), B, T, t_out, Cc,
                                      L.stream_ptr()), "evt_gelu_rows_fwd")
    return out


def channel_norm_gelu(x, gamma, beta, eps, gelu=True):
    """GroupNorm with one channel per group over the frames of [B, T, C] rows (+ GELU), one launch"""
    if x.dim() != 3 or not x.is_contiguous():
        raise L.EvtError(f"channel_norm_gelu: contiguous [B, T, C] expected, got {tuple(x.shape)}")
    B, T, Cc = x.shape
    out = torch.empty_like(x)
    L.check(L.lib().evt_channel_norm_gelu_fwd(L.dt_of(x), L.ptr(x), L.ptr(gamma), L.ptr(beta), float(eps), L.ptr(out), B,
                                              T, Cc, 1 if gelu else 0, L.stream_ptr()), "evt_channel_norm_gelu_fwd")
    return out


FRONT_CHANNELS, FRONT_K, FRONT_STRIDE = 512, 10, 5     # HuBERT's first convolution


def _check_clips(what, x, lens):
    """the clip front end takes fp32 rows [nseq, N] with their lengths"""
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or x.size(0) < 1:
        raise L.EvtError(f"{what}: contiguous float32 rows [nseq, N] expected")
    L.check_lens(what, x, lens)


def front_frames(n):
    """frames of HuBERT's first layer for a row of n samples (0 below 10)"""
    return 0 if n < FRONT_K else (int(n) - FRONT_K) // FRONT_STRIDE + 1


def hubert_front_rows(wav, lens, weight, gamma, beta, eps, dtype):
    """wav [nseq, N] fp32, lens int32 [nseq] (samples) on the GPU; weight fp32 [512, 10] (or the convolution's [512, 1, 10]),
    gamma / beta fp32 [512] -> [nseq, (N - 10) // 5 + 1, 512] of dtype: conv + GroupNorm(512, 512) + GELU per row over the
    row's own frames, zeros behind them (evt_hubert_front_rows; include/evt.h has the definition).  wav is not read at or
    behind a row's length, a row comes out bit for bit as it does alone."""
    _check_clips("hubert_front_rows", wav, lens)
    nseq, n = wav.shape
    if n < FRONT_K:
        raise L.EvtError(f"hubert_front_rows: rows of at least {FRONT_K} samples expected, got {n}")
    for name, t, numel in (("weight", weight, FRONT_CHANNELS * FRONT_K), ("gamma", gamma, FRONT_CHANNELS),
                           ("beta", beta, FRONT_CHANNELS)):
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != wav.device or t.numel() != numel
                or not t.is_contiguous()):
            raise L.EvtError(f"hubert_front_rows: {name} must be contiguous float32 with {numel} elements on {wav.device}")
    code = L.dt_code(dtype)
    ws_floats = L.lib().evt_hubert_front_ws_floats(nseq, n)
    ws = torch.empty(ws_floats, dtype=torch.float32, device=wav.device)
    out = torch.empty(nseq, front_frames(n), FRONT_CHANNELS, dtype=dtype, device=wav.device)
    L.check(L.lib().evt_hubert_front_rows(
        code, wav.data_ptr(), lens.data_ptr(), nseq, n, weight.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps),
        out.data_ptr(), ws.data_ptr(), ws_floats, L.stream_ptr()), "evt_hubert_front_rows")
    return out


def clip_rescale_rows(x, lens):
    """x [nseq, N] fp32 32 kHz clips, lens int32 [nseq] on the GPU -> (f fp32 [nseq, N], q int16 [nseq, N], peak fp32 [nseq]):
    normalize.py:148-153 per row -- rescale_clip's float clip for HuBERT, its int16 clip for 5-wav32k and the row's peak --
    bit for bit numpy's float32 arithmetic, zeros behind a row's length (evt_clip_rescale_rows).  The caller reads `peak`
    to drop rows above 2.2; q saturates where numpy's cast is undefined."""
    _check_clips("clip_rescale_rows", x, lens)
    nseq, n = x.shape
    if n < 1:
        raise L.EvtError("clip_rescale_rows: empty rows")
    f = torch.empty_like(x)
    q = torch.empty(nseq, n, dtype=torch.int16, device=x.device)
    peak = torch.empty(nseq, dtype=torch.float32, device=x.device)
    L.check(L.lib().evt_clip_rescale_rows(
        x.data_ptr(), lens.data_ptr(), nseq, n, f.data_ptr(), q.data_ptr(), peak.data_ptr(), L.stream_ptr()),
        "evt_clip_rescale_rows")
    return f, q, peak


def _check_i32(what, name, t, numel, device):
    if (not torch.is_tensor(t) or t.dtype != torch.int32 or t.device != device or t.numel() != numel
            or not t.is_contiguous()):
        raise L.EvtError(f"{what}: {name} must be a contiguous int32 tensor of {numel} elements on {device}")


def phone_expand_rows(h, src, item_off, n_items, total, out_dtype=torch.float32):
    """h [B, T, C] hidden rows (fp32 or the build's 16-bit type) -> the packed phone-level features of `n_items` items, a
    1-D tensor of C * total elements of out_dtype: item i is the [C, n_i] block at C * item_off[i], its column p - item_off[i]
    the token row src[p] of h.reshape(-1, C) (zeros for src[p] = -1 or outside the rows).  src int32 [total], item_off int32
    [n_items + 1] on h's device.  One launch (evt_phone_expand_rows; include/evt.h has the definition), no
    synchronisation; rows that no column names are not read."""
    if not torch.is_tensor(h) or h.dim() != 3 or not h.is_contiguous() or not h.is_cuda:
        raise L.EvtError("phone_expand_rows: contiguous [B, T, C] rows on the GPU expected")
    B, T, Cc = h.shape
    n_items, total = int(n_items), int(total)
    if Cc % 8 or not 8 <= Cc <= 4096 or B < 1 or T < 1 or not 1 <= n_items <= 65535 or total < 0:
        raise L.EvtError(f"phone_expand_rows: rows {tuple(h.shape)}, {n_items} items, {total} columns are not served")
    _check_i32("phone_expand_rows", "src", src, total, h.device)
    _check_i32("phone_expand_rows", "item_off", item_off, n_items + 1, h.device)
    if torch.is_grad_enabled() and h.requires_grad:
        raise L.EvtError("phone_expand_rows is inference only: run it under torch.no_grad()")
    out = torch.empty(Cc * total, dtype=out_dtype, device=h.device)
    L.check(L.lib().evt_phone_expand_rows(
        L.dt_of(h), h.data_ptr(), B, T, Cc, src.data_ptr(), item_off.data_ptr(), n_items, total, L.dt_code(out_dtype),
        out.data_ptr(), L.stream_ptr()), "evt_phone_expand_rows")
    return out


def bert_embed_ln_rows(ids, lens, word, pos, type_emb, gamma, beta, eps, dtype, token_type_ids=None):
    """ids int32 [B, T] (right-padded), lens int32 [B] on the GPU; word [vocab, C], pos [max_pos, C], type_emb [types, C],
    gamma / beta [C] fp32 -> LayerNorm(word[ids] + pos[t] + type[tt]) as [B, T, C] of dtype, zeros at and behind lens[b]:
    BERT's embeddings in one launch (evt_bert_embed_ln_rows).  Ids outside the table are clamped on the device; a row is
    bit for bit the same in any batch and with any padding."""
    if not torch.is_tensor(ids) or ids.dim() != 2 or not ids.is_cuda:
        raise L.EvtError("bert_embed_ln_rows: ids [B, T] on the GPU expected")
    B, T = ids.shape
    _check_i32("bert_embed_ln_rows", "ids", ids, B * T, ids.device)
    L.check_lens("bert_embed_ln_rows", ids, lens)
    if token_type_ids is not None:
        _check_i32("bert_embed_ln_rows", "token_type_ids", token_type_ids, B * T, ids.device)
    Cc = word.size(-1)
    for name, t, rows in (("word", word, None), ("pos", pos, None), ("type_emb", type_emb, None), ("gamma", gamma, 1),
                          ("beta", beta, 1)):
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != ids.device or not t.is_contiguous()
                or t.size(-1) != Cc or t.dim() != (1 if rows else 2) or t.data_ptr() % 16):
            raise L.EvtError(f"bert_embed_ln_rows: {name} must be contiguous, 16-byte aligned float32 [.., {Cc}] on {ids.device}")
    if B < 1 or T < 1 or T > pos.size(0) or Cc % 4 or not 4 <= Cc <= 8192:
        raise L.EvtError(f"bert_embed_ln_rows: ids {tuple(ids.shape)} with tables of {pos.size(0)} positions x {Cc} are not served")
    out = torch.empty(B, T, Cc, dtype=dtype, device=ids.device)
    L.check(L.lib().evt_bert_embed_ln_rows(
        L.dt_code(dtype), ids.data_ptr(), None if token_type_ids is None else token_type_ids.data_ptr(), lens.data_ptr(), B, T,
        word.data_ptr(), word.size(0), pos.data_ptr(), pos.size(0), type_emb.data_ptr(), type_emb.size(0), gamma.data_ptr(),
        beta.data_ptr(), float(eps), Cc, out.data_ptr(), L.stream_ptr()), "evt_bert_embed_ln_rows")
    return out


SEMANTIC_MAX_D = 1152     # EVT_SEMANTIC_MAX_D


def make_proj_image(weight):
    """ssl_proj.weight [O, C, taps] -> the fp32 image [taps * C, O] evt_semantic_codes_rows reads: row tap * C + c, column o"""
    if not torch.is_tensor(weight) or weight.dim() != 3:
        raise L.EvtError("make_proj_image: a convolution weight [O, C, taps] expected")
    o, c, taps = weight.shape
    return weight.detach().float().permute(2, 1, 0).reshape(taps * c, o).contiguous()


def rvq_norms(embed):
    """ee[k] = |embed[k]|^2 (evt_rvq_norms)"""
    K, D = embed.shape
    ee = torch.empty(K, dtype=torch.float32, device=embed.device)
    L.check(L.lib().evt_rvq_norms(L.ptr(embed), L.ptr(ee), K, D, L.stream_ptr()), "evt_rvq_norms")
    return ee


def semantic_codes_rows(hs, frames, proj_image, bias, embed, ee=None):
    """hs [B, Tmax, D] hidden states (fp32 or the build's 16-bit type, contiguous, on the GPU), frames: B frame counts (a list
    or a tensor; a device tensor costs one read-back) -> (codes, offsets): the packed int64 codes of all rows and the
    int64 [B + 1] exclusive prefix sum of frames[b] // 2 on the device; row b's codes are codes[offsets[b]: offsets[b + 1]].
    proj_image fp32 [2 D, D] (`make_proj_image(ssl_proj.weight)`), bias fp32 [D], embed fp32 [K, D], ee fp32 [K] (computed by
    evt_rvq_norms when None, one more launch).  One upload of the frame counts and offsets and ONE launch of
    evt_semantic_codes_rows (include/evt.h has the definition): the k = 2, stride 2 projection and the nearest code, nothing behind a row's frames read, a row's codes bit for bit those of the row alone."""
    if not torch.is_tensor(hs) or hs.dim() != 3 or not hs.is_cuda or not hs.is_contiguous():
        raise L.EvtError("semantic_codes_rows: contiguous hidden states [B, Tmax, D] on the GPU expected")
    B, Tmax, D = hs.shape
    if torch.is_tensor(frames):
        frames = frames.reshape(-1).tolist()
    frames = [int(t) for t in frames]
    if len(frames) != B:
        raise L.EvtError(f"semantic_codes_rows: {len(frames)} frame counts for {B} rows")
    if B < 1 or Tmax < 1 or D % 64 or not 64 <= D <= SEMANTIC_MAX_D or any(t < 0 or t > Tmax for t in frames):
        raise L.EvtError(f"semantic_codes_rows: rows {tuple(hs.shape)} with frame counts {frames} are not served")
    K = embed.size(0) if torch.is_tensor(embed) and embed.dim() == 2 else 0
    for name, t, shape in (("proj_image", proj_image, (2 * D, D)), ("bias", bias, (D,)), ("embed", embed, (K, D)),
                           ("ee", ee, (K,))):
        if name == "ee" and t is None:
            continue
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != hs.device or tuple(t.shape) != shape
                or not t.is_contiguous() or t.data_ptr() % 16 or K < 1):
            raise L.EvtError(f"semantic_codes_rows: {name} must be contiguous, 16-byte aligned float32 {shape} on {hs.device}")
    if torch.is_grad_enabled() and hs.requires_grad:
        raise L.EvtError("semantic_codes_rows is inference only: run it under torch.no_grad()")
    if ee is None:
        ee = rvq_norms(embed)
    off = [0]
    for t in frames:
        off.append(off[-1] + t // 2)
    total = off[-1]
    # one int32 buffer for one upload: the int64 offsets (as pairs of words) in front, the frame counts behind them
    host = torch.empty(2 * (B + 1) + B, dtype=torch.int32)
    host[: 2 * (B + 1)].view(torch.int64).copy_(torch.tensor(off, dtype=torch.int64))
    host[2 * (B + 1):] = torch.tensor(frames, dtype=torch.int32)
    frames_host = host[2 * (B + 1):]
    dev = host.to(hs.device)
    frames_dev, offsets = dev[2 * (B + 1):], dev[: 2 * (B + 1)].view(torch.int64)
    codes = torch.empty(total, dtype=torch.int64, device=hs.device)
    L.check(L.lib().evt_semantic_codes_rows(
        L.dt_of(hs), hs.data_ptr(), frames_dev.data_ptr(), frames_host.data_ptr(), offsets.data_ptr(), B, Tmax, D, K,
        proj_image.data_ptr(), bias.data_ptr(), embed.data_ptr(), ee.data_ptr(), codes.data_ptr() if total else None, total,
        L.stream_ptr()), "evt_semantic_codes_rows")
    return codes, offsets


POS_CONV_TILE = 256       # EVT_POS_CONV_TILE: frames per block, counted from a row's frame 0
POS_CONV_CG = (16, 32, 48, 64)


def _pos_conv_shape(what, C, groups, k):
    """the shapes evt_pos_conv_pack / evt_pos_conv_rows serve, refused here before a launch"""
    C, groups, k = int(C), int(groups), int(k)
    cg = C // groups if groups > 0 and C % groups == 0 else 0
    if cg not in POS_CONV_CG or not 2 <= k <= 128 or (k * cg) % 32:
        raise L.EvtError(f"{what}: {C} channels in {groups} groups with k = {k} are not served "
                         f"(channels per group in {POS_CONV_CG}, 2 <= k <= 128, k * cg a multiple of 32)")
    return cg


def pos_conv_image(weight, groups, dtype):
    """weight [C, C / groups, k] fp32 on the GPU (the folded weight of the grouped convolution) -> the image
    evt_pos_conv_rows reads: C * (C / groups) * k elements of dtype in MFMA fragment order (evt_pos_conv_pack; one launch,
    once per loaded checkpoint)"""
    if (not torch.is_tensor(weight) or weight.dim() != 3 or weight.dtype != torch.float32 or not weight.is_cuda
            or not weight.is_contiguous() or weight.data_ptr() % 16):
        raise L.EvtError("pos_conv_image: a contiguous, 16-byte aligned float32 weight [C, C / groups, k] on the GPU expected")
    C, cg, k = weight.shape
    if _pos_conv_shape("pos_conv_image", C, groups, k) != cg:
        raise L.EvtError(f"pos_conv_image: weight {tuple(weight.shape)} is not that of {groups} groups")
    image = torch.empty(C * cg * k, dtype=dtype, device=weight.device)
    L.check(L.lib().evt_pos_conv_pack(L.dt_code(dtype), weight.data_ptr(), C, int(groups), k, image.data_ptr(),
                                      L.stream_ptr()), "evt_pos_conv_pack")
    return image


def pos_conv_rows(x, lens, image, bias, groups, k, gelu=True):
    """x [nseq, T, C] rows (fp32 or the build's 16-bit type), lens int32 [nseq] on the GPU or None (every row full), image
    from `pos_conv_image` of x's dtype, bias fp32 [C] or None -> [nseq, T, C]: the grouped same-length convolution (padding
    k // 2, the last frame of an even k dropped) per row over the row's own frames + bias (+ GELU), zeros behind them, ONE
    launch (evt_pos_conv_rows; include/evt.h has the definition).  x is not read at or behind a row's length; a row comes
    out bit for bit as it does alone."""
    if not torch.is_tensor(x) or x.dim() != 3 or not x.is_cuda or not x.is_contiguous() or x.size(0) < 1 or x.size(1) < 1:
        raise L.EvtError("pos_conv_rows: contiguous rows [nseq, T, C] on the GPU expected")
    nseq, T, C = x.shape
    cg = _pos_conv_shape("pos_conv_rows", C, groups, k)
    if nseq > 65535:
        raise L.EvtError(f"pos_conv_rows: {nseq} rows, at most 65535 are served")
    if lens is not None:
        L.check_lens("pos_conv_rows", x, lens)
    if torch.is_grad_enabled() and x.requires_grad:
        raise L.EvtError("pos_conv_rows is inference only: run it under torch.no_grad()")
    if (not torch.is_tensor(image) or image.dtype != x.dtype or image.device != x.device or image.numel() != C * cg * int(k)
            or not image.is_contiguous() or image.data_ptr() % 16):
        raise L.EvtError(f"pos_conv_rows: image must be pos_conv_image's {C * cg * int(k)} elements of {x.dtype} on {x.device}")
    if bias is not None and (not torch.is_tensor(bias) or bias.dtype != torch.float32 or bias.device != x.device
                             or bias.numel() != C or not bias.is_contiguous() or bias.data_ptr() % 16):
        raise L.EvtError(f"pos_conv_rows: bias must be contiguous, 16-byte aligned float32 [{C}] on {x.device}")
    out = torch.empty_like(x)
    L.check(L.lib().evt_pos_conv_rows(
        L.dt_of(x), x.data_ptr(), None if lens is None else lens.data_ptr(), nseq, T, C, int(groups), int(k),
        image.data_ptr(), None if bias is None else bias.data_ptr(), 1 if gelu else 0, out.data_ptr(), L.stream_ptr()),
        "evt_pos_conv_rows")
    return out


MHA_ROWS_QUERY_TILE = 64  # EVT_MHA_ROWS_QUERY_TILE: queries per block, counted from a row's query 0
MHA_ROWS_KEY_TILE = 32    # EVT_MHA_ROWS_KEY_TILE: keys per step of the online softmax, counted from a row's key 0
MHA_ROWS_D = (32, 64)


def _mha_rows_operand(name, t, B):
    """a strided fp32 view [B, T, >= H * D] the C ABI can address: unit channel stride, rows a 16-byte multiple apart,
    item b at b * T rows"""
    if (not torch.is_tensor(t) or t.dim() != 3 or t.dtype != torch.float32 or not t.is_cuda or t.size(0) != B or t.size(1) < 1
            or t.stride(2) != 1 or (B > 1 and t.stride(0) != t.size(1) * t.stride(1))):
        raise L.EvtError(f"mha_rows_f32: {name} must be a float32 [B, T, H * D] view on the GPU with unit channel stride and "
                         "items T rows apart")
    if t.stride(1) % 4 or t.data_ptr() % 16:
        raise L.EvtError(f"mha_rows_f32: {name} rows must be 16-byte aligned and a 16-byte multiple apart")


def mha_rows_f32(q, k, v, lens_q, lens_k, n_heads, scale):
    """q [B, Tq, H * D], k / v [B, Tk, H * D]: strided float32 views (slices of one packed [q | k | v] projection or three
    planes; k and v with one row stride), lens_q / lens_k int32 [B] on the GPU or None (all rows live) -> contiguous
    [B, Tq, H * D]: softmax(scale * q k^T) v per head over each item's live keys, zeros for the query rows at or behind
    lens_q[b] and for items without a live key.  ONE launch of evt_mha_rows_f32 (include/evt.h has the definition): fp32
    MFMA, D in MHA_ROWS_D, nothing at or behind a row's length read, a row bit for bit as it comes out alone."""
    if not torch.is_tensor(q) or q.dim() != 3:
        raise L.EvtError("mha_rows_f32: q [B, Tq, H * D] expected")
    B, Tq, Cc = q.shape
    for name, t in (("q", q), ("k", k), ("v", v)):
        _mha_rows_operand(name, t, B)
        if torch.is_grad_enabled() and t.requires_grad:
            raise L.EvtError("mha_rows_f32 is inference only: run it under torch.no_grad()")
    n_heads = int(n_heads)
    D = Cc // n_heads if n_heads > 0 and Cc % n_heads == 0 else 0
    if D not in MHA_ROWS_D or k.size(2) != Cc or v.shape != k.shape or v.stride(1) != k.stride(1) or B > 65535:
        raise L.EvtError(f"mha_rows_f32: q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)} with {n_heads} heads are not "
                         f"served (head width in {MHA_ROWS_D}, k and v alike)")
    if lens_q is not None:
        L.check_lens("mha_rows_f32", q, lens_q)
    if lens_k is not None:
        L.check_lens("mha_rows_f32", k, lens_k)
    return mha_rows_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), lens_q, lens_k, B, Tq, k.size(1), n_heads, D, q.stride(1),
                           k.stride(1), scale, q.device)


def mha_rows_launch(qp, kp, vp, lens_q, lens_k, B, Tq, Tk, n_heads, D, ldq, ldk, scale, device):
    """the launch of `mha_rows_f32` on device addresses whose shapes the caller has established (hip/enc.py's route on the
    projection buffer it has just written): the output's allocation and the call, nothing else on the host"""
    out = torch.empty(B, Tq, n_heads * D, dtype=torch.float32, device=device)
    prm = L.MhaParams(L.DT_F32, B, n_heads, D, Tq, Tk, -1, 1, ldq, ldk, n_heads * D, float(scale), 0.0, 0, 0, None)
    L.check(L.lib().evt_mha_rows_f32(
        C.byref(prm), qp, kp, vp, None if lens_q is None else lens_q.data_ptr(), None if lens_k is None else lens_k.data_ptr(),
        out.data_ptr(), L.stream_ptr()), "evt_mha_rows_f32")
    return out


GEMM_ROWS_TILE_M = 128    # EVT_GEMM_ROWS_TILE_M: rows per block of the large tile, counted from an item's row 0
GEMM_ROWS_TILE_N = 128    # EVT_GEMM_ROWS_TILE_N
GEMM_ROWS_TILE_K = 32     # EVT_GEMM_ROWS_TILE_K: floats of K per LDS chunk
GEMM_ROWS_ACT_NONE, GEMM_ROWS_ACT_GELU = 0, 1


def gemm_rows_shape(N, K, lda):
    """the shapes evt_gemm_rows_f32 serves (csrc/gemm_rows.hip): whole 16-wide MFMA tiles of columns and of K, rows a
    16-byte multiple apart"""
    return N > 0 and K > 0 and lda > 0 and N % 16 == 0 and K % 16 == 0 and lda % 4 == 0


def conv_rows_weight(weight):
    """a convolution weight [cout, cin, k] -> the fp32 matrix [cout, k * cin] evt_gemm_rows_f32 multiplies with the rows
    of a channels-last buffer: column tap * cin + c (one permute per loaded checkpoint)"""
    if not torch.is_tensor(weight) or weight.dim() != 3:
        raise L.EvtError("conv_rows_weight: a convolution weight [cout, cin, k] expected")
    cout, cin, k = weight.shape
    return weight.detach().float().permute(0, 2, 1).reshape(cout, k * cin).contiguous()


def gemm_rows_f32(x, lens, w, bias, act, rows=None, lda=None, out=None):
    """x: contiguous float32 items [nseq, ...] on the GPU (item b = the floats x[b]), lens int32 [nseq] on the GPU or None
    (every row live), w float32 [N, K], bias float32 [N] or None, act GEMM_ROWS_ACT_NONE / _GELU -> [nseq, rows, N]:
        y[b, m] = act(x[b].flatten()[m * lda: m * lda + K] @ w.T + bias) for m < lens[b], zeros behind,
    ONE launch of evt_gemm_rows_f32 (include/evt.h has the definition).  lda defaults to K (a dense layer over [nseq, T, K]);
    for a channels-last [nseq, T, cin] buffer lda = stride * cin with w = conv_rows_weight(weight) is the convolution without
    padding, rows overlapping.  rows defaults to all that fit an item; out: an optional destination, every element of which
    is written.  Nothing at or behind row lens[b] of an item is read;
    a row comes out bit for bit as it does alone."""
    if not torch.is_tensor(x) or x.dim() < 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise L.EvtError("gemm_rows_f32: contiguous float32 items [nseq, ...] expected")
    if not torch.is_tensor(w) or w.dim() != 2 or w.dtype != torch.float32 or w.device != x.device or not w.is_contiguous():
        raise L.EvtError(f"gemm_rows_f32: w must be a contiguous float32 matrix [N, K] on {x.device}")
    N, K = w.shape
    nseq, item = x.size(0), x[0].numel()
    lda = K if lda is None else int(lda)
    if not gemm_rows_shape(N, K, lda) or item % 4 or not 1 <= nseq <= 65535:
        raise L.EvtError(f"gemm_rows_f32: {nseq} items of {item} floats, rows {lda} apart, with w {tuple(w.shape)} are not served "
                         "(N and K multiples of 16, lda and the item multiples of 4, at most 65535 items)")
    fit = (item - K) // lda + 1 if item >= K else 0
    rows = fit if rows is None else int(rows)
    if not 1 <= rows <= fit:
        raise L.EvtError(f"gemm_rows_f32: {rows} rows of {K} floats, {lda} apart, do not fit an item of {item}")
    if x.data_ptr() % 16 or w.data_ptr() % 16:
        raise L.EvtError("gemm_rows_f32: x and w must be 16-byte aligned")
    if bias is not None and (not torch.is_tensor(bias) or bias.dtype != torch.float32 or bias.device != x.device
                             or bias.numel() != N or not bias.is_contiguous() or bias.data_ptr() % 16):
        raise L.EvtError(f"gemm_rows_f32: bias must be contiguous, 16-byte aligned float32 [{N}] on {x.device}")
    if int(act) not in (GEMM_ROWS_ACT_NONE, GEMM_ROWS_ACT_GELU):
        raise L.EvtError(f"gemm_rows_f32: act {act!r} is neither GEMM_ROWS_ACT_NONE nor GEMM_ROWS_ACT_GELU")
    if lens is not None:
        L.check_lens("gemm_rows_f32", x, lens)
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or (bias is not None and bias.requires_grad)):
        raise L.EvtError("gemm_rows_f32 is inference only: run it under torch.no_grad()")
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != x.device
                            or tuple(out.shape) != (nseq, rows, N) or not out.is_contiguous() or out.data_ptr() % 16):
        raise L.EvtError(f"gemm_rows_f32: out must be contiguous, 16-byte aligned float32 {(nseq, rows, N)} on {x.device}")
    if not x.is_cuda:                                   # last: the checks above are the same for tensors anywhere
        raise L.EvtError("gemm_rows_f32: the items must be on the GPU; there is no CPU path")
    return gemm_rows_launch(x.data_ptr(), lens, w.data_ptr(), None if bias is None else bias.data_ptr(), nseq, rows, N, K, item,
                            lda, int(act), x.device, out=out)


def gemm_rows_launch(xp, lens, wp, bp, nseq, rows, N, K, x_item, lda, act, device, out=None):
    """the launch of `gemm_rows_f32` on device addresses whose shapes the caller has established (the extractors' layers on
    their own parameters): the output's allocation (or `out`, a contiguous float32 [nseq, rows, N] destination such as one
    plane of a q | k | v buffer) and the call, nothing else on the host"""
    if out is None:
        out = torch.empty(nseq, rows, N, dtype=torch.float32, device=device)
    prm = L.GemmRowsParams(nseq, rows, N, K, x_item, lda, act, 0)
    e0 = T.t0()
    L.check(L.lib().evt_gemm_rows_f32(C.byref(prm), xp, None if lens is None else lens.data_ptr(), wp, bp, out.data_ptr(),
                                      L.stream_ptr()), "evt_gemm_rows_f32")
    if e0 is not None:                                  # a traced run (hip/trace.py): every row counted as live
        T.t1(e0, None, "fwd", 2 * nseq * rows * N * K, 4 * (nseq * x_item + N * K + nseq * rows * N),
             f"rows {K}>{N} lda{lda} n{nseq} L{rows}", None)
    return out


def add_layernorm(x, r, gamma, beta, eps):
    """LayerNorm(x + r) over the last axis (r may be None): evt_add_layernorm_fwd, statistics discarded"""
    x = x.contiguous()
    r = r.contiguous() if r is not None else None
    Cc = x.size(-1)
    rows = x.numel() // Cc
    y = torch.empty_like(x)
    stats = torch.empty(2, rows, dtype=torch.float32, device=x.device)
    L.check(L.lib().evt_add_layernorm_fwd(L.dt_of(x), L.ptr(x), L.ptr(r), L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(stats[0]),
                                          L.ptr(stats[1]), rows, Cc, float(eps), L.stream_ptr()),
            "evt_add_layernorm_fwd")
    return y

"""Bindings of the feature extractors' own launches (csrc/feat_ops.hip) and the LayerNorm entry point they share with the s1
blocks.  Inference only: nothing here records an autograd graph."""
import torch

from . import lib as L


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

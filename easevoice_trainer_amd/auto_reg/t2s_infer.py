"""KV-cache decoding of the s1 model: Text2SemanticDecoder.infer_panel_naive,
src/easevoice/soundstorm/auto_reg/models/t2s_model.py:762-863, with T2SBlock.process_prompt / decode_next_token
(:124-222) and sample() (models/utils.py:118-171).

Same token sequence as the reference for the same sampling noise; a different execution plan:
  * prompt pass: the training kernels without gradients (packed qkv GEMM, analytic prefix-LM flash attention, fused
    residual+LayerNorm); its keys/values are copied once into a preallocated cache [layers][B][Lmax][E];
  * token steps: five launches per block (csrc/s1_decode.hip: in-projection, cache attention, out-projection, two for
    the MLP) + logits + one for sampling / embedding / counters, all reading their per-step state (cache length, step
    index, token count) from device memory, captured once into a HIP graph and replayed per token.  The host reads the stop flag every `poll` steps; tokens decoded past the stop are discarded.
  * batches: a session of up to four rows runs the kernels above; 5..32 rows share ONE wide session (one prompt pass,
    one step loop) whose linear layers read every weight once per step for all rows (csrc/s1_decode_rows.hip) and whose
    sampler keys each row's noise by a row-seed table, so a row draws what it drew in a group of four.
  * continuous batching (StreamSession, decode_stream): the counters live per row (csrc/s1_decode_stream.hip), so rows of
    one session have their own prompt length, step index and limit; a finished row's slot is refilled with the next
    waiting text between two graph replays and results are handed out as they finish.  The sampling parameters are per
    row as well (a device table next to the counters), so requests of one session may differ in them, one captured graph
    serves every parameter set, and a request can be cancelled between two polls (StreamControl).  A request may ask
    for n candidates: one prompt pass, n slots, n noise lanes; with logprobs=True the sampler also writes the model's and
    the sampler's log-probability of every drawn token (evt_dec_sample_embed_rows_lp).  A request may carry a forced
    prefix ("force": its first f tokens are given, not drawn -- evt_dec_sample_embed_rows_f) and its own noise seed
    ("seed"); StreamControl.preempt(r) takes a running row out of its slot with the tokens it has, and the two keys
    continue it exactly, here or in another stream; score_stream forces whole sequences and returns their
    log-probabilities.
The reference reads two device scalars per token (the EOS tests of :846) and reallocates every cache tensor per token.

How the module is laid out: _Session owns what every session has -- the buffers, the launch chain of a token step and the
capture of its graph; DecodeSession (shared counters) and StreamSession (per-row counters) add their state, their attention
and their end-of-step launch.  T2SInfer has ONE prompt pass (_prompt_pass: _decode runs it for all rows of a call, _admit
for the slots of an admission) and ONE session cache (_held, behind session / stream_session).  A request of a stream is
parsed once, by _RequestParser, into a Request record that _fits, _stream and _admit read by field name."""
import collections
import ctypes as C
import math
import operator
import os
import time

import torch
from torch.nn import functional as F

from ..hip import lib as L
from ..hip.linear import LinearBank, gemm_fwd
from .ops import AddLayerNormFn, PrefixLMAttentionFn

MAX_STEPS = 1500          # t2s_model.py:822
NO_EOS_STEPS = 11         # t2s_model.py:833


class _Weights:
    """per-block matrices in the streaming dtype (fp32 parameters as they are, or one-time bf16 copies), vectors fp32"""

    def __init__(self, model, dtype):
        self.stamp = self.stamp_of(model)
        cv = (lambda t: t.detach().contiguous()) if dtype == torch.float32 else (lambda t: t.detach().to(dtype).contiguous())
        f32 = lambda t: t.detach().float().contiguous()
        self.layers = []
        for lyr in model.h.layers:
            a = lyr.self_attn
            self.layers.append(dict(
                wqkv=cv(a.in_proj_weight), bqkv=f32(a.in_proj_bias), wo=cv(a.out_proj.weight), bo=f32(a.out_proj.bias),
                w1=cv(lyr.linear1.weight), b1=f32(lyr.linear1.bias), w2=cv(lyr.linear2.weight), b2=f32(lyr.linear2.bias),
                g1=f32(lyr.norm1.weight), be1=f32(lyr.norm1.bias), g2=f32(lyr.norm2.weight), be2=f32(lyr.norm2.bias),
                eps1=float(lyr.norm1.eps), eps2=float(lyr.norm2.eps)))
        self.wpred = cv(model.ar_predict_layer.weight)
        self.emb = f32(model.ar_audio_embedding.word_embeddings.weight)
        self.alpha = f32(model.ar_audio_position.alpha)

    @staticmethod
    def stamp_of(model):
        return tuple(p._version for p in model.parameters()) + tuple(p.data_ptr() for p in model.parameters())


class _Session:
    """what DecodeSession and StreamSession share: the static buffers of B rows, the launch chain of one token step and
    the captured step graph.  A subclass adds its counters, names the library's linear-layer entry point (gemv_fn) and
    supplies _attn(i) and _end_step(W, sp, noise, pe).  The chain looks _gemv, _attn and _end_step up on the session at
    call time, so a function assigned onto a subclass (the CPU emulations of the tests) takes effect."""

    gemv_fn = "evt_dec_gemm_rows"
    fusable = False        # whether step_launches(fused_qkv=True) may put the in-projection into the attention launch

    def __init__(self, model, B, Lmax, ymax, dtype, device):
        self.model, self.B, self.Lmax, self.ymax, self.dtype, self.device = model, B, Lmax, ymax, dtype, device
        E, nl, V = model.model_dim, model.num_layers, model.vocab_size
        self.E, self.H, self.nl, self.V = E, model.num_head, nl, V
        z = self._zeros
        self.kc = z(nl, B, Lmax, E, dt=dtype)
        self.vc = z(nl, B, Lmax, E, dt=dtype)
        self.xa, self.xb = z(B, E), z(B, E)
        self.qkv, self.att, self.t, self.u = z(B, 3 * E), z(B, E), z(B, E), z(B, E)
        self.hid = z(B, 4 * E)
        self.logits = z(B, V)
        self.y = z(B, ymax, dt=torch.int64)
        self.row_seed = z(B, 2, dt=torch.int32)  # (seed, lane) of each row's built-in noise
        self.graph, self.graph_key = None, None

    def _zeros(self, *s, dt=torch.float32):
        return torch.zeros(*s, dtype=dt, device=self.device)

    def _gemv(self, w, bias, a, r, g, b, eps, x_out, y, relu=0):
        N, K = w.shape
        fn = self.gemv_fn
        L.check(getattr(L.lib(), fn)(L.dt_of(w), L.ptr(w), L.ptr(bias), L.ptr(a), L.ptr(r), L.ptr(g), L.ptr(b),
                                     float(eps), L.ptr(x_out), L.ptr(y), self.B, N, K, int(relu), L.stream_ptr()), fn)

    def step_launches(self, W, sp, noise, pe, fused_qkv=False):
        """one token: 24 x (in-projection, cache attention, out-proj, ffn1, ffn2) + logits + the end of the step (sampling
        / embedding / counters: one launch, three in a DecodeSession of several rows) = 122 or 124 launches.  fused_qkv
        puts the in-projection into the attention launch of a session that can (98 launches): 16 workgroups then stream
        all of W_qkv, which is slower on the device (measured 696 vs 614 us per token under graph replay) but faster
        when the HOST is the bottleneck (eager launches: 959 vs 1210 us).  In a StreamSession idle and stopped rows
        ride along in the linear layers on stale inputs; the attention and the sampler skip them."""
        prev = None
        for i, w in enumerate(W.layers):
            ln = (None, None, None, 0.0, None) if prev is None else (self.u, prev["g2"], prev["be2"], prev["eps2"], self.xa)
            src = self.xa if prev is None else self.xb   # later blocks: LayerNorm2 of the previous one, stored to xa
            if fused_qkv and self.fusable:
                self._qkv_attn(i, w, src, *ln)
            else:
                self._gemv(w["wqkv"], w["bqkv"], src, *ln, self.qkv)
                self._attn(i)
            self._gemv(w["wo"], w["bo"], self.att, None, None, None, 0.0, None, self.t)
            self._gemv(w["w1"], w["b1"], self.xa, self.t, w["g1"], w["be1"], w["eps1"], self.xb, self.hid, relu=1)
            self._gemv(w["w2"], w["b2"], self.hid, None, None, None, 0.0, None, self.u)
            prev = w
        self._gemv(W.wpred, None, self.xb, self.u, prev["g2"], prev["be2"], prev["eps2"], None, self.logits)
        self._end_step(W, sp, noise, pe)

    def capture(self, gkey, W, sp, noise, pe, restore=()):
        """the step graph under the key gkey: warm-up launches outside the capture on a side stream, then the capture.
        Both move whatever counters are live, so the tensors of `restore` are put back afterwards (a stream session
        captures with every slot idle and has nothing to restore)."""
        dev = self.device
        keep = [t.clone() for t in restore]
        side = L.role_stream(dev, "decode_warm", ring=1)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self.step_launches(W, sp, noise, pe)
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="relaxed"):
            self.step_launches(W, sp, noise, pe)
        for t, k in zip(restore, keep):
            t.copy_(k)
        self.graph, self.graph_key, self._keep = g, gkey, (sp, noise, pe, W)


class DecodeSession(_Session):
    """a session of rows that share one set of counters ctr (csrc/s1_decode.hip), one per (batch, cache capacity, dtype)"""

    def __init__(self, model, B, Lmax, ymax, dtype, device):
        super().__init__(model, B, Lmax, ymax, dtype, device)
        self.ctr = self._zeros(8, dt=torch.int32)
        self.stop = torch.full((B,), -1, dtype=torch.int32, device=device)
        self.x_lens, self.x_len = None, 0      # key-padding of a batch of texts (infer_panel_batch_infer); None = no padding
        self.x_lens_buf = self._zeros(B, dt=torch.int32)
        # 5..32 rows: evt_dec_gemm_rows / evt_dec_sample_rows with the row_seed table that T2SInfer._decode writes, and
        # never fused: every (row, head) workgroup would stream its head's rows of W_qkv again
        self.wide = B > T2SInfer.MAX_ROWS
        self.gemv_fn, self.fusable = ("evt_dec_gemm_rows", False) if self.wide else ("evt_dec_gemv", True)

    # ---- launches ----
    def _sample_embed_advance(self, W, sp, noise, pe, dpos):
        """sampling, append, embedding of the new token and the counter update: one launch for one sequence, three for a
        batch (the counters may only move after every row's workgroup has read them)"""
        lib = L.lib()
        xs = float(self.model.ar_audio_position.x_scale)
        if self.B == 1:
            L.check(lib.evt_dec_sample_embed(
                C.byref(sp), L.ptr(self.logits), L.ptr(self.y), L.ptr(self.ctr), L.ptr(noise), L.ptr(self.stop),
                L.ptr(W.emb), L.ptr(pe), L.ptr(W.alpha), xs, L.ptr(self.xa), self.E, pe.size(0), dpos, L.stream_ptr()),
                "evt_dec_sample_embed")
            return
        if self.wide:
            L.check(lib.evt_dec_sample_rows(C.byref(sp), L.ptr(self.logits), L.ptr(self.y), L.ptr(self.ctr), L.ptr(noise),
                                            L.ptr(self.stop), None, L.ptr(self.row_seed), self.B, L.stream_ptr()),
                    "evt_dec_sample_rows")
        else:
            L.check(lib.evt_dec_sample(C.byref(sp), L.ptr(self.logits), L.ptr(self.y), L.ptr(self.ctr), L.ptr(noise),
                                       L.ptr(self.stop), None, self.B, L.stream_ptr()), "evt_dec_sample")
        L.check(lib.evt_dec_embed(L.ptr(W.emb), L.ptr(pe), L.ptr(W.alpha), xs, L.ptr(self.y), L.ptr(self.ctr), L.ptr(self.xa),
                                  self.B, self.E, self.ymax, pe.size(0), L.stream_ptr()), "evt_dec_embed")
        L.check(lib.evt_dec_advance(L.ptr(self.ctr), dpos, L.stream_ptr()), "evt_dec_advance")

    def _end_step(self, W, sp, noise, pe):
        self._sample_embed_advance(W, sp, noise, pe, 1)

    def _attn(self, i):
        L.check(L.lib().evt_dec_attn(L.dt_of(self.kc), L.ptr(self.qkv), L.ptr(self.kc[i]), L.ptr(self.vc[i]),
                                     L.ptr(self.ctr), L.ptr(self.att), self.B, self.H, self.E // self.H, self.Lmax,
                                     L.ptr(self.x_lens), self.x_len, L.stream_ptr()), "evt_dec_attn")

    def _qkv_attn(self, i, w, a, r, g, b, eps, x_out):
        L.check(L.lib().evt_dec_qkv_attn(L.dt_of(self.kc), L.ptr(w["wqkv"]), L.ptr(w["bqkv"]), L.ptr(a), L.ptr(r), L.ptr(g),
                                         L.ptr(b), float(eps), L.ptr(x_out), L.ptr(self.kc[i]), L.ptr(self.vc[i]),
                                         L.ptr(self.ctr), L.ptr(self.att), self.B, self.H, self.E // self.H, self.Lmax,
                                         L.ptr(self.x_lens), self.x_len, L.stream_ptr()), "evt_dec_qkv_attn")


ROW_WORDS = 8             # include/evt.h EVT_ROW_*
ROW_POS, ROW_IDX, ROW_YCOUNT, ROW_YLEN, ROW_LIMIT, ROW_STATUS, ROW_NOISE, ROW_NFORCE = range(8)
ROW_IDLE, ROW_RUNNING, ROW_STOP_EOS, ROW_STOP_LIMIT = range(4)


SAMPLE_KEYS = ("top_k", "top_p", "temperature", "repetition_penalty")


# what decode_stream yields when log-probabilities or several candidates per request were asked for: candidate c of
# `request`; y, idx as in the 3-tuple form; logprobs None or fp32 [steps taken][2] (model, sampler), see decode_stream
StreamOutput = collections.namedtuple("StreamOutput", "request y idx candidate logprobs")


class StreamControl:
    """handle of a running decode_stream for the caller that consumes it: cancel(r) withdraws request r, preempt(r)
    takes it out of its slot and hands out the tokens it has so far (decode_stream).  Either only records the index; the
    stream acts at its next poll, so the caller calls them between two next() calls (one thread)."""

    def __init__(self):
        self.cancelled = set()
        self.preempted = set()

    def cancel(self, r):
        self.cancelled.add(int(r))

    def preempt(self, r):
        self.preempted.add(int(r))


class StreamSession(_Session):
    """static buffers + the captured step graph of a continuously batched session: B slots, each with its own counters
    rstate[b] (csrc/s1_decode_stream.hip).  Cache slab of a slot: [0, Xmax) the text, padded and masked by x_lens[b];
    [Xmax, Xmax + ylen[b] + steps) the audio.  All per-row state is device memory, so admitting a text into a free slot
    changes no launch argument; that includes the row's top_k / top_p / temperature / repetition_penalty (row_sample[b]),
    so the graph is captured once per (vocabulary-level parameters, noise table) and serves every parameter set."""

    def __init__(self, model, B, Xmax, Lmax, ymax, dtype, device):
        super().__init__(model, B, Lmax, ymax, dtype, device)
        self.Xmax = Xmax
        z = self._zeros
        self.state = z(B * (ROW_WORDS + 1), dt=torch.int32)      # rstate [B][8], then stop [B]: one read per poll
        self.rstate = self.state[:B * ROW_WORDS].view(B, ROW_WORDS)
        self.stop = self.state[B * ROW_WORDS:]
        self.x_lens = z(B, dt=torch.int32)
        self.row_sample = z(B, 4, dt=torch.int32)                 # evt_row_sample [B]: top_k, then the bits of 3 floats
        self.mask = z(B, dt=torch.int32)                          # rows of an admission's step 0
        self.logp, self.lp_on = None, False                       # [B][ymax][2] of a logprobs=True stream, made on demand
        self.force_on = False                                     # a stream with forced requests: the _f sampler launch
        self.noise_cands = 1                                      # C of an injected [steps][R][C][V] noise table

    def reset(self):
        self.state.zero_()                 # every slot idle
        self.stop.fill_(-1)

    # ---- launches ----
    def _attn(self, i):
        L.check(L.lib().evt_dec_attn_rows(L.dt_of(self.kc), L.ptr(self.qkv), L.ptr(self.kc[i]), L.ptr(self.vc[i]),
                                          L.ptr(self.rstate), L.ptr(self.att), self.B, self.H, self.E // self.H,
                                          self.Lmax, L.ptr(self.x_lens), self.Xmax, L.stream_ptr()), "evt_dec_attn_rows")

    def _sample_embed(self, W, sp, noise, pe, dpos, mask=None):
        """sampling, append, EOS / limit test, next-input embedding and the row's counter update: one launch for all rows
        (each row's workgroup owns its counters); `mask` restricts it to the rows of an admission.  top_k, top_p,
        temperature and repetition_penalty of a row come from row_sample[b]; `sp` carries the session-wide rest.  A
        stream with logprobs=True launches the variant that also fills logp[b][YCOUNT]; a stream with forced requests
        launches the one that takes the token of a row's forced steps from y (with or without logp)"""
        fn = "evt_dec_sample_embed_rows_" + ("f" if self.force_on else "lp" if self.lp_on else "p")
        logp = () if fn.endswith("_p") else (L.ptr(self.logp) if self.lp_on else None,)
        L.check(getattr(L.lib(), fn)(
            C.byref(sp), L.ptr(self.row_sample), L.ptr(self.logits), L.ptr(self.y), L.ptr(self.rstate), L.ptr(noise),
            L.ptr(self.stop), None, L.ptr(self.row_seed), L.ptr(mask), L.ptr(W.emb), L.ptr(pe), L.ptr(W.alpha),
            float(self.model.ar_audio_position.x_scale), L.ptr(self.xa), *logp, self.B, self.E, pe.size(0), dpos,
            L.stream_ptr()), fn)

    def _end_step(self, W, sp, noise, pe):
        self._sample_embed(W, sp, noise, pe, 1)


# one request of a decode_stream as _RequestParser hands it to _fits, _stream and _admit: r its index in the stream,
# limit its number of steps at most, sampling the four values of _sampling, n its candidates, force None or the tokens
# of its forced steps (int64, CPU), seed None or its own (seed, lane)
Request = collections.namedtuple("Request", "r x bert prompt limit sampling n force seed")
# a running slot, and a slot that a poll found finished, cancelled or preempted (kind: "finish", "cancel", "preempt", the
# name of its event)
_Row = collections.namedtuple("_Row", "request ylen candidate")
_Done = collections.namedtuple("_Done", "slot request y idx candidate logprobs kind")


class _RequestParser:
    """(r, request of decode_stream) -> Request, or an EvtError that names the request.  Built from the values of the
    whole stream: `base` the session-wide sampling values by SAMPLE_KEYS, n, slots, early_stop_num, the injected noise
    table or None, and whether the stream is lazy, was opened with forced=True, records log-probabilities."""

    def __init__(self, model, base, n, slots, early_stop_num, noise, lazy, forced, logprobs):
        self.slots, self.early_stop_num, self.lazy, self.forced, self.logprobs = slots, early_stop_num, lazy, forced, logprobs
        self.V, self.eos = model.vocab_size, model.EOS
        self.has_noise = noise is not None
        self.nsteps = None if noise is None else int(noise.size(0))
        self.ncols = None if noise is None or noise.dim() == 2 else int(noise.size(1))
        self.ncand = int(noise.size(2)) if noise is not None and noise.dim() == 4 else None
        self.base_n = self.candidates(n, "decode_stream")
        self.base = base
        self.base_v = T2SInfer._sampling(*base.values(), "decode_stream")
        # the step capacity of a lazy stream is known before its first request is drawn; a list's comes from its requests
        self.cap_steps = self.limit(None) if lazy else None

    def limit(self, early_stop_num):
        lim = T2SInfer._limit(self.early_stop_num if early_stop_num is None else early_stop_num)
        return lim if self.nsteps is None else min(lim, self.nsteps)      # an injected noise table also bounds the steps

    def candidates(self, v, who):
        try:
            if isinstance(v, bool):
                raise TypeError("a bool")
            v = operator.index(v)
        except TypeError:
            raise L.EvtError(f"{who}: n = {v!r} is not an integer") from None
        if not 1 <= v <= self.slots:
            raise L.EvtError(f"{who}: n = {v} must be 1..slots = {self.slots}")
        return v

    def force_of(self, v, who, lim):
        V, eos = self.V, self.eos
        try:
            t = torch.as_tensor(v).detach().cpu()
        except (TypeError, ValueError, RuntimeError) as e:
            raise L.EvtError(f"{who}: force is no token vector ({e})") from None
        if t.dim() != 1 or t.numel() < 1 or t.dtype == torch.bool or t.is_floating_point() or t.is_complex():
            raise L.EvtError(f"{who}: force must be a 1-D integer vector of at least one token")
        t = t.long()
        f = t.numel()
        bad = ((t < 0) | (t >= V)).nonzero()
        if bad.numel():
            j = int(bad[0])
            raise L.EvtError(f"{who}: force[{j}] = {int(t[j])} is outside [0, {V})")
        at = (t == eos).nonzero().reshape(-1).tolist()
        if at and at[0] == 0:
            raise L.EvtError(f"{who}: force[0] is EOS ({eos}), but step 0 has no EOS column")
        if at and at[0] != f - 1:
            raise L.EvtError(f"{who}: force[{at[0]}] is EOS ({eos}) before the last position {f - 1}")
        if f > lim:
            raise L.EvtError(f"{who}: {f} forced tokens, but the request's step limit is {lim}")
        if self.cap_steps is not None and f > self.cap_steps:
            raise L.EvtError(f"{who}: {f} forced tokens, but the session's capacity is {self.cap_steps} steps")
        return t

    @staticmethod
    def seed_of(v, who):
        pair = v if isinstance(v, (tuple, list)) else (v, 0)
        try:
            if len(pair) != 2 or any(isinstance(e, bool) for e in pair):
                raise TypeError("expected an int or a pair (seed, lane) of ints")
            sd, lane = operator.index(pair[0]), operator.index(pair[1])
        except TypeError as e:
            raise L.EvtError(f"{who}: seed = {v!r} is not an integer or (integer, lane) ({e})") from None
        if not 0 <= lane < T2SInfer.MAX_ROWS:
            raise L.EvtError(f"{who}: seed lane = {lane} must be 0..{T2SInfer.MAX_ROWS - 1}")
        return sd & 0x7FFFFFFF, lane

    def __call__(self, r, req):
        if len(req) not in (3, 4):
            raise L.EvtError(f"request {r}: expected (x, bert, prompt[, early_stop_num or dict])")
        x, bert, prompt = req[0].reshape(-1), req[1], req[2].reshape(-1)
        opt, samp, nr = req[3] if len(req) == 4 else None, self.base_v, self.base_n
        force = own_seed = None
        if isinstance(opt, dict):
            unknown = sorted(set(opt) - set(SAMPLE_KEYS) - {"early_stop_num", "n", "force", "seed"})
            if unknown:
                raise L.EvtError(f"request {r}: unknown key(s) {unknown} (known: {list(SAMPLE_KEYS)}, "
                                 "early_stop_num, n, force and seed)")
            if "n" in opt:
                nr = self.candidates(opt["n"], f"request {r}")
            force = opt.get("force")
            if opt.get("seed") is not None:
                own_seed = self.seed_of(opt["seed"], f"request {r}")
            samp = T2SInfer._sampling(*({**self.base, **{k: v for k, v in opt.items() if k in SAMPLE_KEYS}}[k]
                                        for k in SAMPLE_KEYS), f"request {r}")
            opt = opt.get("early_stop_num")
        lim = self.limit(opt)
        if x.numel() < 1 or prompt.numel() < 1:
            raise L.EvtError(f"request {r}: empty text or prompt")
        if self.ncols is not None and r >= self.ncols:
            raise L.EvtError(f"request {r}: the noise table has {self.ncols} columns")
        if nr > 1 and self.has_noise and self.ncand is None:
            raise L.EvtError(f"request {r}: n = {nr}, but the noise table has no candidate dimension "
                             "([steps][R][C][V])")
        if self.ncand is not None and nr > self.ncand:
            raise L.EvtError(f"request {r}: n = {nr}, but the noise table has {self.ncand} candidates per request")
        if self.lazy and nr > 1 and not (self.logprobs or self.base_n > 1):
            raise L.EvtError(f"request {r}: n = {nr} in a lazy stream needs logprobs=True or a session-wide n > 1 "
                             "(the form of the outputs is fixed when the stream is opened)")
        if force is not None:
            if self.lazy and not self.forced:
                raise L.EvtError(f"request {r}: \"force\" in a lazy stream needs decode_stream(..., forced=True) "
                                 "(the sampler launch is fixed when the stream is opened)")
            force = self.force_of(force, f"request {r}", lim)
        return Request(r, x, bert, prompt, lim, samp, nr, force, own_seed)


class T2SInfer:
    """decoder front end bound to one Text2SemanticDecoder; `infer_panel_naive` has the reference's signature"""

    def __init__(self, model):
        self.model = model
        self._w, self._sessions, self._dense = None, {}, None
        self._wide = []            # keys of the wide sessions held, least recently used first

    def weights(self, dtype):
        if self._w is None or self._w[0] != dtype or self._w[1].stamp != _Weights.stamp_of(self.model):
            self._w = (dtype, _Weights(self.model, dtype))
            self._sessions.clear()          # captured graphs hold pointers into the old copies
            self._wide.clear()
        return self._w[1]

    def dense(self, dtype, device):
        """x, weight[, relu] -> act(x W^T + b) for the prompt pass (T2SBlock.process_prompt, t2s_model.py:124-185 of the
        reference: five F.linear per block) on the library's GEMM entry points.  Inside a trainer the model's own
        LinearBank serves (same images as the training forward); a bare model (inference/t2s.py) gets a bank of its own
        here, rebuilt when the weights were replaced or written (load_state_dict)."""
        m = self.model
        bank = getattr(m, "_bank", None)
        if bank is None or bank.dtype != dtype or bank.device != torch.device(device):
            stamp = _Weights.stamp_of(m)
            if self._dense is None or self._dense[0] != (dtype, str(device)) or self._dense[2] != stamp:
                keep = {id(w): getattr(w, "_evt_slot", None) for _n, w, _b in m.dense_specs()}
                own = LinearBank(m.dense_specs(), dtype, device)
                slots = {id(s.weight): s for s in own.slots}
                for _n, w, _b in m.dense_specs():       # a training bank of another dtype keeps its slots on the weights
                    if keep[id(w)] is not None:
                        w._evt_slot = keep[id(w)]
                    else:
                        del w._evt_slot
                self._dense = ((dtype, str(device)), own, stamp, slots)
            bank, slots = self._dense[1], self._dense[3]
        else:
            slots = None
        bank.prepare()

        def run(x, weight, relu=False):
            slot = slots[id(weight)] if slots is not None else weight._evt_slot
            return gemm_fwd(slot, x, relu=relu)

        return run

    def _held(self, make, B, Lneed, yneed, dtype, device, *tag, lru=True, admit=None):
        """the session cache: capacities rounded up to 512; a session under `lru` is one of the WIDE_SESSIONS most
        recently used ones, a dropped one taking its cache and its captured graph with it.  admit(Lmax) may refuse a
        session that has to be made -- after the least recently used one has made room, before anything is allocated or
        recorded"""
        Lmax, ymax = -(-Lneed // 512) * 512, -(-yneed // 512) * 512
        key = (B, Lmax, ymax, dtype, str(device), *tag)
        if lru:
            if key in self._wide:
                self._wide.remove(key)
            else:
                while len(self._wide) >= self.WIDE_SESSIONS:
                    del self._sessions[self._wide.pop(0)]
            if admit is not None and key not in self._sessions:
                admit(Lmax)
            self._wide.append(key)
        if key not in self._sessions:
            self._sessions[key] = make(Lmax, ymax)
        return self._sessions[key]

    def session(self, B, Lneed, yneed, dtype, device):
        """sessions of <= MAX_ROWS rows are kept per shape; of the wide ones (up to 3.2 GB of bf16 cache at B = 32,
        Lmax = 2048) only the WIDE_SESSIONS most recently used"""
        return self._held(lambda Lmax, ymax: DecodeSession(self.model, B, Lmax, ymax, dtype, device),
                          B, Lneed, yneed, dtype, device, lru=B > self.MAX_ROWS)

    def stream_session(self, B, Xmax, Lneed, yneed, dtype, device):
        """the session cache of session(): capacities rounded to 512, stream sessions share the wide-session LRU.  A
        session of more than WIDE_ROWS slots (decode_stream(wide=True)) is refused when its key/value cache,
        2 * layers * B * Lmax * E * itemsize bytes (12.9 GB of bf16 at B = 128, Lmax = 2048), would need more than half
        of the free device memory: before anything is allocated, and with the figures in the message.  Free memory is
        what the device reports plus what torch's allocator holds unused, counted after the least recently used session
        has made room (a refused session therefore still costs that one; it is made again when asked for)"""
        def admit(Lmax):
            if B <= self.WIDE_ROWS or torch.device(device).type != "cuda":
                return
            m = self.model
            need = 2 * m.num_layers * B * Lmax * m.model_dim * torch.empty((), dtype=dtype).element_size()
            free = (torch.cuda.mem_get_info(device)[0] + torch.cuda.memory_reserved(device)
                    - torch.cuda.memory_allocated(device))
            if 2 * need > free:
                raise L.EvtError(f"a stream session of {B} slots and {Lmax} cache positions needs {need} bytes of "
                                 f"key/value cache, more than half of the {free} bytes free on {device}")

        return self._held(lambda Lmax, ymax: StreamSession(self.model, B, Xmax, Lmax, ymax, dtype, device),
                          B, Lneed, yneed, dtype, device, "stream", Xmax, admit=admit)

    MAX_ROWS = 4        # rows of a session on the kernels of csrc/s1_decode.hip (kMaxB); also the seed group of a row
    WIDE_ROWS = 32      # rows of a wide session (csrc/s1_decode_rows.hip); larger batches run in groups of 32
    WIDE_SESSIONS = 2   # wide sessions kept at once
    STREAM_ROWS = 128   # slots of a stream session opened with wide=True: four row groups of evt_dec_gemm_rows

    def _prompt_pass(self, S, W, xs, berts, prompts, y_lens, x_len, rows, spread=lambda t: t):
        """the prompt pass (t2s_model.py:575-660 / 775-825, T2SBlock.process_prompt) of k texts: xs k id vectors, berts
        k x [1024, n], prompts [k, P] (padded to a common length, y_lens the true ones) or None; every text is padded to
        x_len positions, masked as keys.  The keys/values of the k rows go into rows `rows` of S's cache, through
        `spread` when one prompt row serves several cache rows.  Returns the activations after the last block
        [k, x_len + P, E] and the two length vectors on the device."""
        m = self.model
        dev, cd = S.device, S.dtype
        dense = self.dense(cd, dev)           # the library's GEMMs on prepared weight images (hip/linear.py), no vendor BLAS
        embs = []
        for x, bert in zip(xs, berts):
            x, bert = x.to(dev), bert.to(dev)
            xe = m.ar_text_embedding(x.unsqueeze(0))
            xe = xe + dense(bert.transpose(0, 1).unsqueeze(0).to(cd).contiguous(), m.bert_proj.weight).to(xe.dtype)
            xe = m.ar_text_position(xe).squeeze(0)
            embs.append(F.pad(xe, (0, 0, 0, x_len - xe.size(0))))
        xy = torch.stack(embs, dim=0)
        if prompts is not None:
            xy = torch.cat([xy, m.ar_audio_position(m.ar_audio_embedding(prompts))], dim=1)
        xy = xy.to(cd).contiguous()
        src_len = xy.size(1)
        xl = torch.tensor([int(x.numel()) for x in xs], dtype=torch.int32, device=dev)
        yl = torch.tensor(y_lens, dtype=torch.int32, device=dev)
        for i, lyr in enumerate(m.h.layers):
            w = W.layers[i]
            qkv = dense(xy, lyr.self_attn.in_proj_weight)
            S.kc[i, rows, :src_len] = spread(qkv[..., S.E:2 * S.E])
            S.vc[i, rows, :src_len] = spread(qkv[..., 2 * S.E:])
            o = PrefixLMAttentionFn.apply(qkv, xl, yl, x_len, S.H, 0.0, 0)
            sa = dense(o.contiguous(), lyr.self_attn.out_proj.weight)
            xy = AddLayerNormFn.apply(xy, sa, w["g1"], w["be1"], w["eps1"])
            ff = dense(dense(xy.contiguous(), lyr.linear1.weight, relu=True), lyr.linear2.weight)
            xy = AddLayerNormFn.apply(xy, ff, w["g2"], w["be2"], w["eps2"])
        return xy, xl, yl

    @torch.no_grad()
    def _decode(self, xs, berts, prompts, no_eos_steps, top_k, top_p, early_stop_num, temperature, repetition_penalty,
                noise=None, seed=None, poll=8):
        """xs: B id vectors (any lengths), berts: B x [1024, n_b], prompts [B, y_len] or None.  Returns (token buffer
        [B, >= y_len + steps] on the device, per-row index of the last sampled step, per-row EOS flag, y_len)."""
        m = self.model
        if m.training:
            raise L.EvtError("decoding needs model.eval() (the reference decodes with dropout off)")
        dev, cd = xs[0].device, m.cd
        L.set_half(cd)                        # a 16-bit streaming dtype selects the build of the library that serves it
        B = len(xs)
        W = self.weights(cd)
        x_lens = [int(x.numel()) for x in xs]
        x_len = max(x_lens)
        y_len = 0 if prompts is None else prompts.size(1)
        src_len = x_len + y_len
        n_max = self._limit(early_stop_num)
        noise_rows = 1
        if noise is not None:       # an injected noise table (parity runs) also bounds the number of steps
            noise = noise.to(dev, torch.float32).contiguous()
            noise_rows = 1 if noise.dim() == 2 else noise.size(1)
            assert noise.size(-1) == m.vocab_size and noise_rows in (1, B)
            n_max = min(n_max, noise.size(0))
        S = self.session(B, src_len + n_max + 1, y_len + n_max + 1, cd, dev)
        xy, xl, _yl = self._prompt_pass(S, W, xs, berts, prompts, [y_len] * B, x_len, slice(None))
        # ---- state ----
        S.y.zero_()
        if prompts is not None:
            S.y[:, :y_len].copy_(prompts)
        # the sampling seed is device state like the counters (a new one per call must not force a re-capture); without
        # an explicit seed it is drawn from torch's CPU generator, so torch.manual_seed makes a run repeatable.  A wide
        # session gives row b what row b % 4 of a group of four drew: group g seeded seed + 4g, or the g-th draw
        G = self.MAX_ROWS
        draws = [int(seed + G * g if seed is not None else torch.randint(0, 2 ** 31 - 1, (1,)).item()) & 0x7FFFFFFF
                 for g in range(-(-B // G) if S.wide else 1)]
        if S.wide:
            S.row_seed.copy_(torch.tensor([[draws[b // G], b % G] for b in range(B)], dtype=torch.int32))
        S.ctr.copy_(torch.tensor([src_len, 0, y_len, y_len, draws[0], 0, 0, 0], dtype=torch.int32))
        S.stop.fill_(-1)
        padded = min(x_lens) < x_len
        if padded:
            S.x_lens_buf.copy_(xl)
        S.x_lens, S.x_len = (S.x_lens_buf if padded else None), x_len
        sp = L.SampleParams(S.V, m.EOS, int(top_k) if top_k is not None else 0, no_eos_steps, S.ymax, float(top_p),
                            float(temperature), float(repetition_penalty), 0x5EED5EED, noise_rows)
        pe = m.ar_audio_position.pe(max(4000, y_len + n_max + 1), dev, torch.float32).contiguous()
        # ---- step 0: logits of the last prompt position, sample, embed ----
        S.xb.copy_(xy[:, -1].float())
        S._gemv(W.wpred, None, S.xb, None, None, None, 0.0, None, S.logits)
        S._sample_embed_advance(W, sp, noise, pe, 0)
        # ---- token steps: one graph replay each ----
        from .. import hip_graphs_safe

        use_graph = os.environ.get("EVT_DECODE_GRAPH", "1") != "0" and hip_graphs_safe()
        gkey = (bytes(sp), None if noise is None else noise.data_ptr(), pe.data_ptr(), id(W), padded, x_len)
        if use_graph and S.graph_key != gkey:
            S.capture(gkey, W, sp, noise, pe, restore=(S.ctr, S.y, S.stop, S.xa))
        done = 1
        stop = S.stop.tolist() if n_max == 1 else [-1] * B
        while done < n_max and min(stop) < 0:
            if use_graph:
                S.graph.replay()
            else:
                S.step_launches(W, sp, noise, pe, fused_qkv=True)
            done += 1
            if done % poll == 0 or done == n_max:
                stop = S.stop.tolist()              # the only device->host read of the loop
        eos = [s >= 0 for s in stop]
        last = [s if s >= 0 else n_max - 1 for s in stop]   # else: early_stop_num reached, or 1500 steps without EOS
        return S.y, last, eos, y_len

    def infer_panel_naive(self, x, x_lens, prompts, bert_feature, top_k=-100, top_p=100, early_stop_num=-1,
                          temperature=1.0, repetition_penalty=1.35, noise=None, seed=None, poll=8, **kwargs):
        """t2s_model.py:762-863: one sequence; returns (y without its last token, idx - 1), or (.., 0) without a prompt"""
        if x.size(0) != 1:
            raise L.EvtError("one sequence per call (infer_panel_naive_batched loops over the items, t2s_model.py:732-760)")
        ybuf, last, _eos, y_len = self._decode([x[0]], [bert_feature[0]], prompts, NO_EOS_STEPS, top_k, top_p, early_stop_num,
                                               temperature, repetition_penalty, noise=noise, seed=seed, poll=poll)
        y = ybuf[:, :y_len + last[0]].clone()       # the last sampled token (EOS or the stop token) is dropped
        if prompts is None:
            return y.to(torch.int32), 0
        return y, last[0] - 1

    def infer_panel_naive_batched(self, x, x_lens, prompts, bert_feature, **kw):
        ys, idxs = [], []
        for i in range(len(x)):
            y, idx = self.infer_panel_naive(x[i].unsqueeze(0), x_lens[i], prompts[i].unsqueeze(0) if prompts is not None
                                            else None, bert_feature[i].unsqueeze(0), **kw)
            ys.append(y[0])
            idxs.append(idx)
        return ys, idxs

    def infer_panel_batch_infer(self, x, x_lens, prompts, bert_feature, top_k=-100, top_p=100, early_stop_num=-1,
                                temperature=1.0, repetition_penalty=1.35, noise=None, seed=None, poll=8, **kwargs):
        """t2s_model.py:563-730, the TTS default (parallel_infer=True): texts of different lengths decoded together.
        x: list of id vectors, bert_feature: list of [1024, n].  Rows are independent (padded text positions are masked
        as keys, a finished row only leaves the batch), so instead of compacting the batch whenever a row meets EOS, all
        rows of a group keep stepping through the same graph and each row's tokens are cut at its own stop.  Up to
        WIDE_ROWS texts are one group (one prompt pass, one session), more run in groups of WIDE_ROWS.  Kept
        differences to infer_panel_naive: the EOS column is dropped at step 0 only, the returned index is idx - 1 for an
        EOS stop and idx for the early stop.  `seed` (or torch's CPU generator) gives row r the noise of row r % 4 of a
        group seeded seed + 4 * (r // 4), as when every four rows were decoded on their own."""
        if prompts is None:
            return self.infer_panel_naive_batched(x, x_lens, prompts, bert_feature, top_k=top_k, top_p=top_p,
                                                  early_stop_num=early_stop_num, temperature=temperature, noise=noise,
                                                  seed=seed, poll=poll)
        ys, idxs = [], []
        step = self.WIDE_ROWS if len(x) > self.MAX_ROWS else self.MAX_ROWS
        for g0 in range(0, len(x), step):
            rows = list(range(g0, min(len(x), g0 + step)))
            nz = noise if noise is None or noise.dim() == 2 else noise[:, rows]
            ybuf, last, eos, y_len = self._decode([x[r] for r in rows], [bert_feature[r] for r in rows], prompts[rows], 1,
                                                  top_k, top_p, early_stop_num, temperature, repetition_penalty, noise=nz,
                                                  seed=None if seed is None else seed + g0, poll=poll)
            for k in range(len(rows)):
                ys.append(ybuf[k, :y_len + last[k]].clone())
                idxs.append(last[k] - 1 if eos[k] else last[k])
        return ys, idxs

    # ---- continuous batching: finished rows are refilled from a queue (csrc/s1_decode_stream.hip) ----
    @staticmethod
    def _limit(early_stop_num):
        return MAX_STEPS if early_stop_num == -1 else max(1, min(MAX_STEPS, int(early_stop_num) + 1))

    @staticmethod
    def _sampling(top_k, top_p, temperature, repetition_penalty, who):
        """the four sampling values as the table holds them: int(top_k) (None: 0, off), three floats; non-finite values
        and repetition_penalty <= 0 are refused here, the kernel's launcher cannot see the device table"""
        try:
            v = (int(top_k) if top_k is not None else 0, float(top_p), float(temperature), float(repetition_penalty))
        except (TypeError, ValueError, OverflowError) as e:
            raise L.EvtError(f"{who}: bad sampling parameter ({e})") from None
        for name, f in zip(SAMPLE_KEYS[1:], v[1:]):
            if not math.isfinite(f):
                raise L.EvtError(f"{who}: {name} = {f} is not finite")
        if v[3] <= 0.0:
            raise L.EvtError(f"{who}: repetition_penalty = {v[3]} must be > 0")
        return v

    def decode_stream(self, requests, slots=32, top_k=-100, top_p=100, temperature=1.0, repetition_penalty=1.35,
                      early_stop_num=-1, noise=None, seed=None, poll=8, max_text_len=None, max_prompt_len=None,
                      control=None, n=1, logprobs=False, forced=False, wide=False):
        """Continuous batching of infer_panel_batch_infer's decoding.  requests: an iterable of (x, bert, prompt) or
        (x, bert, prompt, opt) -- x a 1-D id vector, bert [1024, n], prompt a 1-D token vector; prompts may differ in
        content and length.  opt is the request's early_stop_num, or a dict with keys out of top_k, top_p, temperature,
        repetition_penalty, early_stop_num that replace the session-wide values for this request alone (an unknown key,
        a non-finite value or repetition_penalty <= 0 raises EvtError naming the request, before anything is launched
        for it).  control: a StreamControl; control.cancel(r) between two next() calls withdraws request r at the next
        poll -- a running row is set idle and its slot freed for the admission that follows, a waiting request is
        skipped without a prompt pass, either is yielded as (r, None, None); a request that finished at that poll is
        delivered.  Returns a generator of (request_index, y, idx) in COMPLETION order, y and idx as
        infer_panel_batch_infer returns them per text.  Up to `slots` (1..32; 1..128 with wide=True, see below) texts
        decode at once in one graph-replayed session; every `poll` steps the rows' status is read, finished rows are
        handed out and their slots refilled
        with the next waiting requests (one prompt pass for all of them).  A list has the capacity (longest text,
        longest prompt, largest limit) computed from itself; a lazy iterable needs max_text_len / max_prompt_len and
        is bounded by `early_stop_num`.  A request that does not fit raises EvtError before anything is launched for
        it.  Request r draws the built-in noise of (seed + 4 * (r // 4), r % 4), the convention of
        infer_panel_batch_infer; an injected table [steps][R][V] is read at column r ([steps][V]: by every request).
        One stream at a time per model and capacity: the session's buffers are shared.

        n: candidates per request (1..slots; a request's dict may carry "n" for itself).  The n candidates of a request
        are admitted together after ONE prompt pass, whose keys/values are copied into n slots; the queue stays FIFO, so
        a head request waits until n slots are free and nothing overtakes it.  Candidate c of request r draws lane
        r % 4 + 4c of the group seed of r: candidate 0 is what n = 1 gives.  An injected table may be
        [steps][R][C][V], candidate c of request r reading [.., r, c, :]; a table without that dimension serves n = 1
        only.  logprobs=True: the sampler also records, per drawn token, the log-softmax of the raw logits at the token
        and the log of the probability it was drawn from (after penalty, nucleus, top-k, temperature).  With
        logprobs=True or any n > 1 the generator yields StreamOutput(request, y, idx, candidate, logprobs) instead of
        3-tuples, exactly n per request (y = idx = logprobs = None for a cancelled candidate); logprobs is None when
        not asked for, else fp32 [last + 1, 2]: rows 0 .. len(y) - prompt_len - 1 belong to y[prompt_len:], the last
        row to the step that stopped the candidate.  A lazy iterable fixes the form when it is opened: there a
        request's own "n" > 1 needs logprobs=True or a session-wide n > 1.

        A request's dict may also carry
          "force": a 1-D integer tensor or list of f >= 1 tokens that the request's first f steps TAKE instead of
            drawing (all n candidates: n continuations of one given prefix).  The step index counts through them, so
            step f reads noise row f.  A forced step stops the row only when its given token is EOS (allowed at the
            last position alone, never at position 0: step 0 has no EOS column); the model's arg-max is not asked.
            With logprobs=True a forced step reports the model's log-probability of the given token and the log of
            the probability the sampler would have drawn it from (-inf when the sampler had cut it).  A token outside
            [0, V), a misplaced EOS, f above the request's step limit or the session's capacity raise EvtError naming
            the request.  A stream with any forced request runs evt_dec_sample_embed_rows_f; a list is inspected as a
            whole, a lazy iterable says forced=True when it is opened (else a drawn request with "force" is refused).
          "seed": an int s -- the row draws the built-in noise of (s & 0x7FFFFFFF, lane 0) -- or a pair (s, lane) with
            lane in 0..3; candidate c adds 4c to the lane as ever.  (S + 4 * (r0 // 4), r0 % 4) draws what request r0
            of a stream seeded S draws, whatever the request's own index, slot or admission time.
        control.preempt(r): at the next poll every running, unfinished candidate of r is set idle as by cancel, but is
        yielded with what it has: y = the row's prompt and tokens so far, idx = None (idx None with y not None marks a
        preempted row), logprobs = those of the steps taken.  A candidate that finished at that poll is delivered, a
        request still waiting at that poll is yielded as cancelled when its turn comes.  Submitting
        (x, bert, prompt, {"force": y[len(prompt):], "seed": ...}) to this or a later stream continues the row exactly
        where it was.

        wide=True allows slots up to STREAM_ROWS = 128: the linear layers run the rows in groups of 32 on one more grid
        dimension, and a row's tokens do not depend on the number of slots.  It is asked for, not silently given,
        because the session's cache grows with the slots: 2 * layers * slots * Lmax * E * itemsize bytes, 12.9 GB in
        bf16 and 25.8 GB in fp32 at 128 slots and Lmax = 2048, and WIDE_SESSIONS of them are kept.  A session of more
        than 32 slots that would need more than half of the free device memory is refused with an EvtError."""
        if self.model.training:
            raise L.EvtError("decoding needs model.eval() (the reference decodes with dropout off)")
        most = self.STREAM_ROWS if wide else self.WIDE_ROWS
        if not 1 <= int(slots) <= most:
            raise L.EvtError(f"slots must be 1..{most}, got {slots}")
        slots, logprobs, forced = int(slots), bool(logprobs), bool(forced)
        lazy = not isinstance(requests, (list, tuple))
        parse = _RequestParser(self.model, dict(zip(SAMPLE_KEYS, (top_k, top_p, temperature, repetition_penalty))), n,
                               slots, early_stop_num, noise, lazy, forced, logprobs)
        rich = logprobs or parse.base_n > 1
        if not lazy:
            reqs = [parse(r, q) for r, q in enumerate(requests)]
            if not reqs:
                return iter(())
            rich = rich or any(q.n > 1 for q in reqs)
            forced = forced or any(q.force is not None for q in reqs)
            Xmax = int(max_text_len) if max_text_len is not None else max(q.x.numel() for q in reqs)
            Pmax = int(max_prompt_len) if max_prompt_len is not None else max(q.prompt.numel() for q in reqs)
            cap = (Xmax, Pmax, max(q.limit for q in reqs))
            for q in reqs:
                self._fits(q, cap)
            it = iter(reqs)
        else:
            if max_text_len is None or max_prompt_len is None:
                raise L.EvtError("a lazy iterable of requests needs max_text_len and max_prompt_len (the session's "
                                 "capacity is fixed when it is made)")
            cap = (int(max_text_len), int(max_prompt_len), parse.cap_steps)
            it = (parse(r, q) for r, q in enumerate(requests))
        return self._stream(it, cap, slots, top_k, top_p, temperature, repetition_penalty, noise, seed,
                            max(1, int(poll)), control, logprobs, rich, forced)

    def score_stream(self, requests, tokens, slots=32, append_eos=False, wide=False, **sampling):
        """Log-probabilities of GIVEN tokens: request r = (x, bert, prompt[, opt]) is forced over all of tokens[r] (a 1-D
        integer vector; append_eos=True adds EOS behind it), limited to exactly that many steps, with logprobs=True.
        Yields (r, logprobs) in completion order, logprobs fp32 [f, 2]: per given token the model's log-probability and
        the log of the probability the sampler would have drawn it from under the request's sampling values (-inf where
        the sampler cuts the token).  No noise value can change a forced row, so `seed` / `noise` do not matter; the
        other keywords are decode_stream's.  A thin wrapper over decode_stream: the sequence is scored by the decode
        steps themselves, one token per step, with the sampler's own arithmetic."""
        eos = self.model.EOS

        def forced_requests():
            for r, (req, tok) in enumerate(zip(requests, tokens)):
                try:
                    t = torch.as_tensor(tok).detach().cpu().reshape(-1)
                except (TypeError, ValueError, RuntimeError) as e:
                    raise L.EvtError(f"request {r}: tokens are no vector ({e})") from None
                if append_eos and not t.is_floating_point():
                    t = torch.cat([t.long(), torch.tensor([eos])])
                opt = req[3] if len(req) == 4 else None
                opt = dict(opt) if isinstance(opt, dict) else {}
                opt.update(force=t, early_stop_num=max(0, t.numel() - 1))      # _limit: exactly t.numel() steps
                yield (req[0], req[1], req[2], opt)

        lazy = not isinstance(requests, (list, tuple))
        reqs = forced_requests() if lazy else list(forced_requests())
        for o in self.decode_stream(reqs, slots=slots, logprobs=True, forced=True, wide=wide, **sampling):
            yield o.request, o.logprobs

    @staticmethod
    def _fits(q, cap):
        if q.x.numel() > cap[0] or q.prompt.numel() > cap[1] or q.limit > cap[2]:
            raise L.EvtError(f"request {q.r} (text {q.x.numel()}, prompt {q.prompt.numel()}, {q.limit} steps) does not fit the "
                             f"session's capacity (text {cap[0]}, prompt {cap[1]}, {cap[2]} steps)")

    @torch.no_grad()
    def _stream_open(self, cap, slots, dev, top_k, top_p, temperature, repetition_penalty, noise, logprobs=False,
                     forced=False):
        """session, weights, sampling parameters and the captured step graph; every slot idle"""
        m = self.model
        cd = m.cd
        L.set_half(cd)
        W = self.weights(cd)
        Xmax, Pmax, n_max = cap
        noise_rows, cands = 1, 1
        if noise is not None:
            noise = noise.to(dev, torch.float32).contiguous()
            if noise.dim() == 4:      # [steps][R][C][V]: candidate c of request r reads the flattened column r * C + c
                cands, noise = noise.size(2), noise.flatten(1, 2)
            noise_rows = 1 if noise.dim() == 2 else noise.size(1)
            assert noise.size(-1) == m.vocab_size
        S = self.stream_session(slots, Xmax, Xmax + Pmax + n_max + 1, Pmax + n_max + 1, cd, dev)
        S.reset()
        S.lp_on, S.noise_cands, S.force_on = bool(logprobs), cands, bool(forced)
        if S.lp_on and S.logp is None:
            S.logp = torch.zeros(S.B, S.ymax, 2, dtype=torch.float32, device=dev)
        sp = L.SampleParams(S.V, m.EOS, int(top_k) if top_k is not None else 0, 1, S.ymax, float(top_p),
                            float(temperature), float(repetition_penalty), 0x5EED5EED, noise_rows)
        pe = m.ar_audio_position.pe(max(4000, Pmax + n_max + 1), dev, torch.float32).contiguous()
        from .. import hip_graphs_safe

        use_graph = os.environ.get("EVT_DECODE_GRAPH", "1") != "0" and hip_graphs_safe()
        # the four per-request values reach the sampler through S.row_sample, not through sp: the graph does not depend
        # on them
        gkey = (sp.V, sp.eos, sp.no_eos_steps, sp.ymax, sp.seed, sp.noise_rows,
                None if noise is None else noise.data_ptr(), pe.data_ptr(), id(W))
        if S.lp_on:      # another sampler kernel in the graph; a session without it keeps the key it always had
            gkey = gkey + ("logprobs",)
        if S.force_on:   # likewise: the sampler launch with forced steps
            gkey = gkey + ("force",)
        captured = bool(use_graph and S.graph_key != gkey)
        if captured:
            # every slot is idle here: the warm-up and the capture move no counter and write no cache line, so there is
            # no state to restore (the activations they leave are overwritten by each admission)
            S.capture(gkey, W, sp, noise, pe)
        return S, W, sp, pe, noise, use_graph, captured

    @torch.no_grad()
    def _admit(self, S, W, sp, pe, noise, batch, seeds):
        """batch: [(slots, Request)], `slots` the n slots of the request's candidates in candidate order.  The prompt
        pass for these requests only, ONE row per request (texts padded to Xmax, prompts to the longest of them); each
        row's keys/values go into the cache slabs of all its slots, then the row state of every slot and step 0 for
        those slots: logits of the last prompt position and a masked sample."""
        dev = S.device
        Xmax, k = S.Xmax, len(batch)
        y_lens = [int(q.prompt.numel()) for _s, q in batch]
        Pk = max(y_lens)
        pr = torch.stack([F.pad(q.prompt.to(dev).long(), (0, Pk - q.prompt.numel())) for _s, q in batch], dim=0)
        # per slot: (prompt row it copies from, candidate number, its request); one entry per request when every n is 1
        per = [(i, c, q) for i, (sl, q) in enumerate(batch) for c in range(len(sl))]
        slots_t = torch.tensor([s for sl, _q in batch for s in sl], dtype=torch.long, device=dev)
        if len(per) == k:
            spread = lambda t: t
        else:
            src_t = torch.tensor([i for i, _c, _q in per], dtype=torch.long, device=dev)
            spread = lambda t: t[src_t]
        xy, xl, yl = self._prompt_pass(S, W, [q.x for _s, q in batch], [q.bert for _s, q in batch], pr, y_lens, Xmax,
                                       slots_t, spread)
        # ---- row state ----
        # noise column: none for a [steps][V] table, the request's for [steps][R][V]; `noise` arrives with a candidate
        # dimension flattened ([steps][R * C][V], _stream_open), C = S.noise_cands: column r * C + c
        C_ = S.noise_cands
        ncol = (lambda r, c: 0) if noise is None or noise.dim() == 2 else (lambda r, c: r * C_ + c)
        # word 7: the row's forced steps; their tokens go behind the prompt in y, where the sampler launch finds them
        rs = [[Xmax + y_lens[i], 0, y_lens[i], y_lens[i], q.limit, ROW_RUNNING, ncol(q.r, c),
               0 if q.force is None else q.force.numel()] for i, c, q in per]
        S.rstate[slots_t] = torch.tensor(rs, dtype=torch.int32).to(dev)
        S.stop[slots_t] = -1
        # candidate c draws lane r % 4 + 4c of the request's group seed (the hash folds the lane in as lane << 16): at
        # most 3 + 4 * 127 = 511 with n = STREAM_ROWS candidates, well inside the 16 bits the hash gives the lane
        own = [q.seed if q.seed is not None else seeds(q.r) for _i, _c, q in per]      # a request's own (seed, lane)
        S.row_seed[slots_t] = torch.tensor([[sd, lane + self.MAX_ROWS * c] for (sd, lane), (_i, c, _q) in zip(own, per)],
                                           dtype=torch.int32).to(dev)
        tab = torch.tensor([[0.0, *q.sampling[1:]] for _i, _c, q in per], dtype=torch.float32)
        tab.view(torch.int32)[:, 0] = torch.tensor([q.sampling[0] for _i, _c, q in per], dtype=torch.int32)
        S.row_sample[slots_t] = tab.view(torch.int32).to(dev)      # moved as integers: every bit pattern survives
        S.x_lens[slots_t] = spread(xl)
        S.y[slots_t] = 0
        S.y[slots_t, :Pk] = spread(pr)
        for (sl, q), P in zip(batch, y_lens):
            if q.force is not None:
                S.y[torch.tensor(sl, device=dev), P:P + q.force.numel()] = q.force.to(dev)
        S.mask.zero_()
        S.mask[slots_t] = 1
        # ---- step 0 of the admitted rows (the other rows' xb / logits are dead between two steps) ----
        S.xb[slots_t] = spread(xy[torch.arange(k, device=dev), Xmax + yl.long() - 1].float())
        S._gemv(W.wpred, None, S.xb, None, None, None, 0.0, None, S.logits)
        S._sample_embed(W, sp, noise, pe, 0, S.mask)

    def _stream(self, it, cap, slots, top_k, top_p, temperature, repetition_penalty, noise, seed, poll, control=None,
                logprobs=False, rich=False, forced=False):
        G, draws = self.MAX_ROWS, []

        def seeds(r):          # (seed, lane) of request r: group r // 4 seeded seed + 4 * (r // 4), or its own draw
            g = r // G
            while len(draws) <= g:
                draws.append(int(seed + G * len(draws) if seed is not None
                                 else torch.randint(0, 2 ** 31 - 1, (1,)).item()) & 0x7FFFFFFF)
            return draws[g], r % G

        stats = self.stream_stats = dict(steps=0, admissions=0, admitted=[], prefill_rows=[], prefill_s=[], events=[],
                                         graph_captured=False)
        free, running, S, exhausted = list(range(slots)), {}, None, False
        left = {}              # per running slot: graph replays until its row must have stopped
        cancelled = control.cancelled if control is not None else ()
        preempted = getattr(control, "preempted", ()) if control is not None else ()
        due = set()            # preempt() calls seen at a poll so far: a request still waiting then comes back as cancelled
        out = (lambda r, y, idx, c, lp: StreamOutput(r, y, idx, c, lp)) if rich else (lambda r, y, idx, c, lp: (r, y, idx))
        head = None            # the request at the head of the queue, drawn but still waiting for its n slots
        while True:
            batch = []
            while free and (head is not None or not exhausted):
                if head is None:
                    try:
                        head = next(it)
                    except StopIteration:
                        exhausted = True
                        break
                    self._fits(head, cap)
                q = head
                if q.r in cancelled or q.r in due:     # withdrawn while it waited: no prompt pass, no slot
                    head = None
                    stats["events"].append(("cancel", stats["steps"], q.r, None))
                    for c in range(q.n):
                        yield out(q.r, None, None, c, None)
                    continue
                if q.n > len(free):             # FIFO: it waits for its n slots and nothing overtakes it
                    break
                head = None
                batch.append(([free.pop(0) for _ in range(q.n)], q))
            if batch:
                dev = batch[0][1].x.device
                if S is None:
                    S, W, sp, pe, noise, use_graph, stats["graph_captured"] = self._stream_open(
                        cap, slots, dev, top_k, top_p, temperature, repetition_penalty, noise, logprobs, forced)
                cuda = torch.device(dev).type == "cuda"
                if cuda:
                    torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                self._admit(S, W, sp, pe, noise, batch, seeds)
                if cuda:
                    torch.cuda.synchronize(dev)
                stats["prefill_s"].append(time.perf_counter() - t0)
                stats["admissions"] += 1
                stats["admitted"].append(sum(len(sl) for sl, _q in batch))
                stats["prefill_rows"].append(len(batch))
                for sl, q in batch:
                    for c, slot in enumerate(sl):
                        running[slot], left[slot] = _Row(q.r, int(q.prompt.numel()), c), q.limit - 1
                        stats["events"].append(("admit", stats["steps"], q.r, slot))
            if not running:
                return
            n = min(poll, max(left.values()))
            for _ in range(n):
                if use_graph:
                    S.graph.replay()
                else:
                    with torch.no_grad():
                        S.step_launches(W, sp, noise, pe)
            stats["steps"] += n
            st = S.state.tolist()                    # the only device->host read of the loop: status and stop of all rows
            done = []
            due.update(preempted)
            for slot in sorted(running):
                r, ylen, c = running[slot]
                left[slot] = max(0, left[slot] - n)
                status = st[slot * ROW_WORDS + ROW_STATUS]
                if status in (ROW_STOP_EOS, ROW_STOP_LIMIT):
                    last = st[S.B * ROW_WORDS + slot]
                    # one pair per step 0..last, written at the index the step's token went to: y[ylen + step]
                    lp = S.logp[slot, ylen:ylen + last + 1].clone() if logprobs else None
                    done.append(_Done(slot, r, S.y[slot, :ylen + last].clone(),
                                      last - 1 if status == ROW_STOP_EOS else last, c, lp, "finish"))
                elif r in cancelled:
                    # an ordinary write on the stream of the replays: the row's workgroups see IDLE from the next
                    # replay on and return at once, whatever an admission later makes of the slot
                    S.rstate[slot, ROW_STATUS] = ROW_IDLE
                    done.append(_Done(slot, r, None, None, c, None, "cancel"))
                elif r in due:
                    # idle as above; the row's tokens and log-probabilities up to the YCOUNT of this poll's state read
                    # are cloned on the stream of the replays, before an admission can write the slot
                    S.rstate[slot, ROW_STATUS] = ROW_IDLE
                    yc = st[slot * ROW_WORDS + ROW_YCOUNT]
                    lp = S.logp[slot, ylen:yc].clone() if logprobs else None
                    done.append(_Done(slot, r, S.y[slot, :yc].clone(), None, c, lp, "preempt"))
            if n == 0 and not done:
                raise L.EvtError("stream session: a row is past its step limit but not stopped")
            for d in done:
                del running[d.slot], left[d.slot]
                free.append(d.slot)
                stats["events"].append((d.kind, stats["steps"], d.request, d.slot))
            free.sort()
            for d in done:
                yield out(d.request, d.y, d.idx, d.candidate, d.logprobs)

    def infer_panel_batch_infer_refill(self, x, x_lens, prompts, bert_feature, slots=32, top_k=-100, top_p=100,
                                       early_stop_num=-1, temperature=1.0, repetition_penalty=1.35, noise=None, seed=None,
                                       poll=8, logprobs=False, wide=False, **kwargs):
        """infer_panel_batch_infer on a refilled session: the same arguments and the same (ys, idxs) in input order, but
        the texts go through `slots` rows of ONE session, a finished row's slot taking the next text, instead of groups
        of 32 that each wait for their slowest row.  prompts: [R, P] or a list of 1-D token vectors of any lengths.
        top_k, top_p, temperature, repetition_penalty and early_stop_num: a scalar for all texts, or a sequence with
        one value per text.  logprobs=True returns (ys, idxs, lps), lps[r] the fp32 [steps, 2] log-probabilities of text
        r as decode_stream hands them out.  `slots` is first clamped to the number of texts (no slot would stay idle),
        then checked by decode_stream: 1..32, with wide=True 1..128 -- so a larger value passes when there are no more
        texts than that, as slots=33 always did."""
        if prompts is None:
            if logprobs:
                raise L.EvtError("logprobs needs prompts (the refilled session)")
            return self.infer_panel_naive_batched(x, x_lens, prompts, bert_feature, top_k=top_k, top_p=top_p,
                                                  early_stop_num=early_stop_num, temperature=temperature, noise=noise,
                                                  seed=seed, poll=poll)
        R = len(x)
        given = dict(top_k=top_k, top_p=top_p, temperature=temperature, repetition_penalty=repetition_penalty,
                     early_stop_num=early_stop_num)
        per = {k: list(v) for k, v in given.items()
               if isinstance(v, (list, tuple)) or (torch.is_tensor(v) and v.dim() > 0)}
        for k, v in per.items():
            if len(v) != R:
                raise L.EvtError(f"{k}: {len(v)} values for {R} texts")
            v[:] = [e.item() if torch.is_tensor(e) else e for e in v]
        base = {k: (per[k][0] if k in per and R else v) for k, v in given.items()}     # per-text values replace these
        if per:
            reqs = [(x[r], bert_feature[r], prompts[r], {k: v[r] for k, v in per.items()}) for r in range(R)]
        else:
            reqs = [(x[r], bert_feature[r], prompts[r]) for r in range(R)]
        ys, idxs, lps = [None] * len(reqs), [None] * len(reqs), [None] * len(reqs)
        for o in self.decode_stream(reqs, slots=min(int(slots), max(1, len(reqs))), noise=noise, seed=seed, poll=poll,
                                    logprobs=logprobs, wide=wide, **base):
            ys[o[0]], idxs[o[0]] = o[1], o[2]
            if logprobs:
                lps[o[0]] = o.logprobs
        return (ys, idxs, lps) if logprobs else (ys, idxs)

"""TEST-ONLY shim: the continuously batched s1 decode session (auto_reg/t2s_infer.py StreamSession) with its HIP launches
substituted by torch CPU arithmetic on the session's own buffers and PER-ROW counters.  It pins the host side --
admission into free slots, the prompt pass of the admitted requests, row state, polling, hand-out order, refill --
against the reference's token sequences without a GPU.  The prompt pass and the graph switch are emulated as in
cpu_emu.cpu_emulation_decode, which this builds on."""
import contextlib

import torch
import torch.nn.functional as F

from cpu_emu import cpu_emulation_decode
from oracle import s1_step as OS


@contextlib.contextmanager
def cpu_emulation_stream():
    from easevoice_trainer_amd.auto_reg import t2s_infer as TI

    SS = TI.StreamSession
    saved = (SS._gemv, SS._attn, SS._sample_embed)
    POS, IDX, YCOUNT, YLEN, LIMIT, STATUS, NOISE = (TI.ROW_POS, TI.ROW_IDX, TI.ROW_YCOUNT, TI.ROW_YLEN, TI.ROW_LIMIT,
                                                    TI.ROW_STATUS, TI.ROW_NOISE)

    def gemv(self, w, bias, a, r, g, b, eps, x_out, y, relu=0):
        x = a if r is None else F.layer_norm(a + r, (a.size(-1),), g, b, eps)
        if r is not None and x_out is not None:
            x_out.copy_(x)
        o = x @ w.float().t() + (bias if bias is not None else 0.0)
        y.copy_(o.clamp(min=0) if relu else o)

    def attn(self, i):
        """evt_dec_attn_rows: per running row, append at its own position and attend over its own length"""
        E, H = self.E, self.H
        d = E // H
        for b in range(self.B):
            rs = self.rstate[b].tolist()
            if rs[STATUS] != TI.ROW_RUNNING:
                continue
            pos = rs[POS]
            assert 0 <= pos < self.Lmax
            self.kc[i, b, pos] = self.qkv[b, E:2 * E]
            self.vc[i, b, pos] = self.qkv[b, 2 * E:]
            keep = torch.ones(pos + 1, dtype=torch.bool)
            keep[int(self.x_lens[b]):self.Xmax] = False
            K = self.kc[i, b, :pos + 1].float().view(pos + 1, H, d).transpose(0, 1)
            V = self.vc[i, b, :pos + 1].float().view(pos + 1, H, d).transpose(0, 1)
            q = self.qkv[b, :E].view(H, 1, d)
            s = (q @ K.transpose(-1, -2) / d ** 0.5).masked_fill(~keep[None, None, :], float("-inf"))
            self.att[b] = (F.softmax(s, -1) @ V).reshape(E)

    def sample_embed(self, W, sp, noise, pe, dpos, mask=None):
        """evt_dec_sample_embed_rows: every step quantity comes from the row"""
        for b in range(self.B):
            if mask is not None and int(mask[b]) == 0:
                continue
            rs = self.rstate[b].tolist()
            if rs[STATUS] != TI.ROW_RUNNING:
                continue
            idx, ycount, ylen = rs[IDX], rs[YCOUNT], rs[YLEN]
            Ve = sp.V - 1 if idx < sp.no_eos_steps else sp.V
            lg = self.logits[b:b + 1, :Ve].clone()
            prev = self.y[b:b + 1, :ycount]
            if sp.repetition_penalty != 1.0 and ycount > 0:
                sc = torch.gather(lg, 1, prev)
                lg.scatter_(1, prev, torch.where(sc < 0, sc * sp.repetition_penalty, sc / sp.repetition_penalty))
            probs = OS.logits_to_probs(lg, None, sp.temperature, sp.top_k if sp.top_k > 0 else None, sp.top_p, 1.0)
            assert noise is not None, "the CPU emulation has no built-in noise"
            q = noise[idx, rs[NOISE], :Ve] if noise.dim() == 3 else noise[idx, :Ve]
            tok = int(torch.argmax(probs / q, dim=-1)[0])
            self.y[b, ycount] = tok
            self.xa[b] = W.emb[tok] * self.model.ar_audio_position.x_scale + W.alpha * pe[ylen + idx]
            if int(torch.argmax(lg, dim=-1)[0]) == sp.eos or tok == sp.eos:
                self.stop[b] = idx
                self.rstate[b, STATUS] = TI.ROW_STOP_EOS
            elif idx + 1 >= rs[LIMIT]:
                self.stop[b] = idx
                self.rstate[b, STATUS] = TI.ROW_STOP_LIMIT
            else:
                self.rstate[b, POS] += dpos
                self.rstate[b, IDX] += 1
                self.rstate[b, YCOUNT] += 1

    with cpu_emulation_decode():
        SS._gemv, SS._attn, SS._sample_embed = gemv, attn, sample_embed
        try:
            yield
        finally:
            SS._gemv, SS._attn, SS._sample_embed = saved

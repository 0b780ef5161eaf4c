"""TEST-ONLY shim: cpu_emu_stream_lp.cpu_emulation_stream_lp with the launch of evt_dec_sample_embed_rows_f emulated as
well.  When the session runs with forced requests (StreamSession.force_on), a running row b whose step index is below
rstate[b][NFORCE] does not sample: its token is the one the admission wrote at y[b][YCOUNT].  With torch on the
session's buffers the row gets
    x[b] = emb[token] * x_scale + alpha * pe[YLEN + IDX], the append, the counters and the limit test as ever,
    STOP_EOS only when the given token is EOS (the arg-max rule is off in a forced step),
    logp[b][YCOUNT][0] = log_softmax(logits[b, :Ve])[token]                              (with lp_on)
    logp[b][YCOUNT][1] = log(probs[token]), probs as the emulated sampler forms them: -inf for a token it had cut.
Rows that are not in a forced step go through cpu_emulation_stream_lp unchanged, and so does a session without force_on.
"""
import contextlib

import torch

from cpu_emu_stream_lp import cpu_emulation_stream_lp
from oracle import s1_step as OS


@contextlib.contextmanager
def cpu_emulation_stream_force():
    from easevoice_trainer_amd.auto_reg import t2s_infer as TI

    SS = TI.StreamSession
    with cpu_emulation_stream_lp():
        inner = SS._sample_embed

        def sample_embed(self, W, sp, noise, pe, dpos, mask=None):
            if not self.force_on:
                return inner(self, W, sp, noise, pe, dpos, mask)
            st = self.rstate.tolist()
            on = [mask is None or int(mask[b]) != 0 for b in range(self.B)]
            given = [on[b] and st[b][TI.ROW_STATUS] == TI.ROW_RUNNING and st[b][TI.ROW_IDX] < st[b][TI.ROW_NFORCE]
                     for b in range(self.B)]
            rest = torch.tensor([1 if on[b] and not given[b] else 0 for b in range(self.B)], dtype=torch.int32)
            logits = self.logits.clone()
            inner(self, W, sp, noise, pe, dpos, rest)
            ks = self.row_sample[:, 0].tolist()
            fl = self.row_sample.view(torch.float32).tolist()
            for b in range(self.B):
                if not given[b]:
                    continue
                idx, ycount, ylen, limit = (st[b][k] for k in (TI.ROW_IDX, TI.ROW_YCOUNT, TI.ROW_YLEN, TI.ROW_LIMIT))
                tok = int(self.y[b, ycount])
                assert 0 <= tok < sp.V, "the host validates forced tokens"
                self.xa[b] = W.emb[tok] * self.model.ar_audio_position.x_scale + W.alpha * pe[ylen + idx]
                if self.lp_on:
                    Ve = sp.V - 1 if idx < sp.no_eos_steps else sp.V
                    raw = logits[b:b + 1, :Ve]
                    lg = raw.clone()
                    prev = self.y[b:b + 1, :ycount]
                    pen = fl[b][3]
                    if pen != 1.0 and ycount > 0:
                        sc = torch.gather(lg, 1, prev)
                        lg.scatter_(1, prev, torch.where(sc < 0, sc * pen, sc / pen))
                    probs = OS.logits_to_probs(lg, None, fl[b][2], ks[b] if ks[b] > 0 else None, fl[b][1], 1.0)
                    inside = tok < Ve
                    self.logp[b, ycount, 0] = torch.log_softmax(raw, -1)[0, tok] if inside else float("-inf")
                    self.logp[b, ycount, 1] = torch.log(probs[0, tok]) if inside else float("-inf")
                if tok == sp.eos:
                    self.stop[b] = idx
                    self.rstate[b, TI.ROW_STATUS] = TI.ROW_STOP_EOS
                elif idx + 1 >= limit:
                    self.stop[b] = idx
                    self.rstate[b, TI.ROW_STATUS] = TI.ROW_STOP_LIMIT
                else:
                    self.rstate[b, TI.ROW_POS] += dpos
                    self.rstate[b, TI.ROW_IDX] += 1
                    self.rstate[b, TI.ROW_YCOUNT] += 1

        SS._sample_embed = sample_embed
        try:
            yield
        finally:
            SS._sample_embed = inner

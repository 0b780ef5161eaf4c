"""TEST-ONLY shim: cpu_emu_stream_rows.cpu_emulation_stream_rows with the launch of evt_dec_sample_embed_rows_lp emulated
as well.  When the session runs with log-probabilities (StreamSession.lp_on), every row that the emulated sampler is
about to advance gets, from the session's own logits with torch,
    logp[b][YCOUNT][0] = log_softmax(logits[b, :Ve])[token]                                  (the model's)
    logp[b][YCOUNT][1] = log(probs[token]), probs as the emulated sampler forms them         (the sampler's)
with YCOUNT read before the row's counters move.  Without lp_on it is cpu_emulation_stream_rows unchanged."""
import contextlib

import torch

from cpu_emu_stream_rows import cpu_emulation_stream_rows
from oracle import s1_step as OS


@contextlib.contextmanager
def cpu_emulation_stream_lp():
    from easevoice_trainer_amd.auto_reg import t2s_infer as TI

    SS = TI.StreamSession
    with cpu_emulation_stream_rows():
        rows = SS._sample_embed

        def sample_embed(self, W, sp, noise, pe, dpos, mask=None):
            if not self.lp_on:
                return rows(self, W, sp, noise, pe, dpos, mask)
            before = self.rstate.clone()
            logits = self.logits.clone()
            rows(self, W, sp, noise, pe, dpos, mask)
            ks = self.row_sample[:, 0].tolist()
            fl = self.row_sample.view(torch.float32).tolist()
            for b in range(self.B):
                rs = before[b].tolist()
                if (mask is not None and int(mask[b]) == 0) or rs[TI.ROW_STATUS] != TI.ROW_RUNNING:
                    continue
                idx, ycount = rs[TI.ROW_IDX], rs[TI.ROW_YCOUNT]
                Ve = sp.V - 1 if idx < sp.no_eos_steps else sp.V
                tok = int(self.y[b, ycount])
                raw = logits[b:b + 1, :Ve]
                lg = raw.clone()
                prev = self.y[b:b + 1, :ycount]
                pen = fl[b][3]
                if pen != 1.0 and ycount > 0:
                    sc = torch.gather(lg, 1, prev)
                    lg.scatter_(1, prev, torch.where(sc < 0, sc * pen, sc / pen))
                probs = OS.logits_to_probs(lg, None, fl[b][2], ks[b] if ks[b] > 0 else None, fl[b][1], 1.0)
                self.logp[b, ycount, 0] = torch.log_softmax(raw, -1)[0, tok]
                self.logp[b, ycount, 1] = torch.log(probs[0, tok])

        SS._sample_embed = sample_embed
        try:
            yield
        finally:
            SS._sample_embed = rows

"""TEST-ONLY shim: cpu_emu_stream.cpu_emulation_stream with the sampler reading every row's top_k / top_p / temperature /
repetition_penalty from the session's device table row_sample[b], as evt_dec_sample_embed_rows_p does.  The emulated
launch of cpu_emu_stream is called once per row with a copy of `sp` that carries the row's values and a one-row mask."""
import contextlib

import torch

from cpu_emu_stream import cpu_emulation_stream


@contextlib.contextmanager
def cpu_emulation_stream_rows():
    from easevoice_trainer_amd.auto_reg import t2s_infer as TI
    from easevoice_trainer_amd.hip import lib as L

    SS = TI.StreamSession
    with cpu_emulation_stream():
        session_wide = SS._sample_embed

        def sample_embed(self, W, sp, noise, pe, dpos, mask=None):
            ks = self.row_sample[:, 0].tolist()
            fl = self.row_sample.view(torch.float32).tolist()
            for b in range(self.B):
                if mask is not None and int(mask[b]) == 0:
                    continue
                spb = L.SampleParams.from_buffer_copy(sp)
                spb.top_k, spb.top_p, spb.temperature, spb.repetition_penalty = ks[b], fl[b][1], fl[b][2], fl[b][3]
                one = torch.zeros(self.B, dtype=torch.int32)
                one[b] = 1
                session_wide(self, W, spb, noise, pe, dpos, one)

        SS._sample_embed = sample_embed
        try:
            yield
        finally:
            SS._sample_embed = session_wide

"""Loading a trained s2 export for the inference-side entry points.

Mirrors TTS.init_vits_weights (src/easevoice/inference/tts.py:265-299): the export written by SovitsTrain._save_epoch is
`{"weight": fp16 state_dict without enc_q.*, "config": hps, "info": ...}`; the model is rebuilt from `config`, enc_q is
dropped, the weights are loaded non-strictly and the module is put in eval mode.  On top of that the conv weight bank of
the HIP kernels (runtime.ModelRuntime) is built and folded once, since inference never updates the parameters."""
import torch

from ..hip import lib as L
from ..module import models
from ..runtime import ModelRuntime


class SoVITSVoice:
    """`decode(codes, text, refer, noise_scale, speed)` and `extract_latent(ssl)` of SynthesizerTrn (models.py:974-1018)
    on a loaded export, and `decode_batch` for a ragged batch of fragments."""

    def __init__(self, weights, device="cuda:0", dtype=torch.bfloat16):
        ck = torch.load(weights, map_location="cpu", weights_only=False) if isinstance(weights, str) else weights
        hps = ck["config"]
        if hasattr(hps, "model_dump"):
            hps = hps.model_dump()
        if ck["weight"]["enc_p.text_embedding.weight"].shape[0] == 322:
            raise ValueError("The model is version v1, please use the latest version model.")
        self.hps = hps
        d = hps["data"]
        self.sampling_rate, self.hop_length = d["sampling_rate"], d["hop_length"]
        self.filter_length, self.win_length = d["filter_length"], d["win_length"]
        net = models.SynthesizerTrn(d["filter_length"] // 2 + 1, hps["train"]["segment_size"] // d["hop_length"],
                                    n_speakers=d["n_speakers"], **hps["model"])
        del net.enc_q                      # not part of the export, not used by decode
        net.load_state_dict({k: v.float() for k, v in ck["weight"].items()}, strict=False)
        net.eval()
        net.sampling_rate = self.sampling_rate
        self.rt = ModelRuntime(net, dtype=dtype, device=device)
        self.rt.prepare(force=True)
        self.model, self.device, self.dtype = net, torch.device(device), dtype

    @torch.no_grad()
    def decode(self, codes, text, refer, noise_scale=0.5, speed=1, noise=None, style=None):
        """style: a precomputed voice [1, gin] (style_rows, inference/voice.py::enroll_voices) in place of refer (then None)"""
        L.set_half(self.dtype)
        mv = lambda t: t.to(self.device)
        if style is not None:
            return self.model.decode(mv(codes), mv(text), refer, noise_scale=noise_scale, speed=speed,
                                     noise=None if noise is None else mv(noise), style=style)
        refer = [mv(r) for r in refer] if isinstance(refer, (list, tuple)) else mv(refer)
        return self.model.decode(mv(codes), mv(text), refer, noise_scale=noise_scale, speed=speed,
                                 noise=None if noise is None else mv(noise))

    @torch.no_grad()
    def decode_batch(self, codes, code_lens, text, text_lens, refer, noise_scale=0.5, noise=None, speed=1, out_rate=None,
                     out_format=None, interval=0.0, style=None):
        """SynthesizerTrn.decode_batch: a ragged batch of fragments in one pass -> a list of B 1-D waveforms, row b what
        decode gives for fragment b alone (at speed, or at speed[b] where a sequence of B speeds is given); with out_rate /
        out_format a hip.audio.PackedAudio: the rows at that rate and format in one device buffer.  style: precomputed
        voices [1, gin] or [B, gin] on the device in place of refer (then None)"""
        L.set_half(self.dtype)
        mv = lambda t: t.to(self.device)
        mvr = lambda r: None if r is None else [mvr(e) for e in r] if isinstance(r, (list, tuple)) else mv(r)
        if style is not None:
            return self.model.decode_batch(mv(codes), code_lens, mv(text), text_lens, mvr(refer), noise_scale=noise_scale,
                                           noise=None if noise is None else mv(noise), speed=speed, out_rate=out_rate,
                                           out_format=out_format, interval=interval, style=style)
        return self.model.decode_batch(mv(codes), code_lens, mv(text), text_lens, mvr(refer), noise_scale=noise_scale,
                                       noise=None if noise is None else mv(noise), speed=speed, out_rate=out_rate,
                                       out_format=out_format, interval=interval)

    @torch.no_grad()
    def style_rows(self, spec_cl, lens):
        """SynthesizerTrn.style_rows: a ragged batch of channels-last reference spectrograms -> [B, gin] in one pass"""
        L.set_half(self.dtype)
        return self.model.style_rows(spec_cl.to(self.device), lens)

    @torch.no_grad()
    def extract_latent(self, ssl):
        L.set_half(self.dtype)
        return self.model.extract_latent(ssl.to(self.device))

    @torch.no_grad()
    def extract_latent_rows(self, hs, frames):
        """SynthesizerTrn.extract_latent_rows: hidden states [B, Tmax, 768] as CNHubert.last_hidden_state_batch leaves them
        (on this voice's device, fp32 or 16-bit) + B frame counts -> a list of B 1-D int64 code tensors from one launch"""
        L.set_half(hs.dtype if torch.is_tensor(hs) and L.is_half(hs.dtype) else self.dtype)
        return self.model.extract_latent_rows(hs, frames)

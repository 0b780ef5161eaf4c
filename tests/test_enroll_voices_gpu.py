"""GPU: inference/voice.py::enroll_voices -- three voices of 3.0 / 4.1 / 10.0 s, the second with an aux clip, through one
spectrogram launch pair, one pass of the style encoder, one resampling launch and one prompt pass.  CN-HuBERT is a stub with
a deterministic last_hidden_state_batch (the real chain has its own tests: tests/test_hubert_rows_gpu.py); the voice is the
fixture model of the decode tests.  Asserted: styles equal style_rows on ref_spec_rows of the same clips, the aux voice's
style is the mean of its two vectors, prompt tokens equal prompt_semantics on the same 16 kHz clips, a 2.9 s main clip
raises OSError, and clips16k are used as given."""
import json
import os

import pytest
import torch

from util_fill import fill_module

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SECONDS = [3.0, 4.1, 10.0]
AUX_SECONDS = 1.5              # one further clip of voice 1


class StubHubert:
    """frames as CN-HuBERT counts them ((n - 400) // 320 + 1); frame t is a fixed row of a table scaled by the mean
    magnitude of its 320 samples: a deterministic function of the clip that differs between clips"""

    def __init__(self, device):
        self.device = device
        self.table = torch.randn(64, 768, generator=torch.Generator().manual_seed(31)).to(device)
        self.seen = []

    def last_hidden_state_batch(self, clips):
        clips = [torch.as_tensor(c, dtype=torch.float32).reshape(-1).to(self.device) for c in clips]
        self.seen.append([c.clone() for c in clips])
        lens = [(c.numel() - 400) // 320 + 1 for c in clips]
        hs = torch.zeros(len(clips), max(lens), 768, device=self.device)
        for b, (c, t) in enumerate(zip(clips, lens)):
            level = c[:t * 320].view(t, 320).abs().mean(1, keepdim=True)
            hs[b, :t] = self.table[torch.arange(t, device=self.device) % 64] * (1.0 + 4.0 * level)
        return hs, lens


def _clip(seconds, rate, seed, peak):
    n = int(round(seconds * rate))
    x = torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 2 - 1
    return (x * peak * torch.linspace(0.2, 1.0, n)).float()


@pytest.fixture(scope="module")
def enrolled(gpu):
    from easevoice_trainer_amd.inference.sovits import SoVITSVoice
    from easevoice_trainer_amd.inference.voice import enroll_voices
    from easevoice_trainer_amd.module import models

    hps = json.load(open(os.path.join(ROOT, "configs", "s2.json")))
    net = models.SynthesizerTrn(1025, 32, n_speakers=300, **hps["model"])
    fill_module(net, 1)
    weight = {k: v.detach().clone() for k, v in net.state_dict().items() if "enc_q" not in k}
    voice = SoVITSVoice({"weight": weight, "config": hps, "info": "fixture"}, device=str(gpu), dtype=torch.bfloat16)
    clips = [_clip(s, 32000, 40 + i, p) for i, (s, p) in enumerate(zip(SECONDS, (0.7, 1.6, 2.5)))]
    aux = [[], [_clip(AUX_SECONDS, 32000, 50, 0.9)], []]
    hubert = StubHubert(gpu)
    voices = enroll_voices(voice, hubert, clips, aux=aux)
    return voice, hubert, clips, aux, voices


def _padded(rows, gpu):
    lens = [c.numel() for c in rows]
    x = torch.zeros(len(rows), max(lens))
    for b, c in enumerate(rows):
        x[b, :lens[b]] = c
    return x.to(gpu), lens


def test_styles_equal_style_rows_on_ref_spec_rows(gpu, enrolled):
    from easevoice_trainer_amd.hip.audio import ref_spec_rows

    voice, _hubert, clips, aux, voices = enrolled
    x, lens = _padded(clips + aux[1], gpu)
    spec, frames, peak = ref_spec_rows(x, lens)
    assert frames == [n // 640 for n in lens] == [150, 205, 500, 75] and tuple(spec.shape) == (4, 500, 704)
    assert torch.equal(peak.cpu(), torch.stack([c.abs().max() for c in clips + aux[1]]))
    ge = voice.style_rows(spec, frames)
    assert ge.dtype == torch.float32 and tuple(ge.shape) == (4, 512)      # _style's dtype
    assert len(voices) == 3 and [v.frames for v in voices] == [150, 205, 500]
    for v in (0, 2):
        assert tuple(voices[v].style.shape) == (1, 512) and torch.equal(voices[v].style, ge[v:v + 1]), v
    # the aux voice: the mean of its two vectors, taken as decode takes the mean of a list of references
    want = torch.stack([ge[1:2], ge[3:4]], 0).mean(0)
    assert torch.equal(voices[1].style, want)
    assert not torch.equal(voices[1].style, ge[1:2])


def test_prompt_tokens_equal_prompt_semantics_on_the_same_clips(gpu, enrolled):
    from easevoice_trainer_amd.hip.audio import resample_pack
    from easevoice_trainer_amd.inference.semantic import PROMPT_TAIL, prompt_semantics

    voice, hubert, clips, _aux, voices = enrolled
    x, lens = _padded(clips, gpu)
    packed = resample_pack(x, lens, 1, 32000, 16000, "float32")
    assert packed.lengths == [48000, 65600, 160000]
    clips16 = [packed.row(b).clone() for b in range(3)]
    # the stub was called once, with exactly these clips and the reference's 0.3 s of zeros behind each
    assert len(hubert.seen) == 1 and len(hubert.seen[0]) == 3
    for got, c in zip(hubert.seen[0], clips16):
        assert got.numel() == c.numel() + PROMPT_TAIL and torch.equal(got[:c.numel()], c) and bool((got[c.numel():] == 0).all())
    want = prompt_semantics(StubHubert(gpu), voice.extract_latent, clips16)
    for v in range(3):
        t = voices[v].prompt_semantic
        assert t.dim() == 1 and t.dtype == torch.long and torch.equal(t, want[v]), v
    assert not torch.equal(want[0], want[1][:want[0].numel()])          # the stub's tokens do depend on the clip


def test_short_main_clip_raises_and_aux_may_be_short(gpu, enrolled):
    from easevoice_trainer_amd.inference.voice import enroll_voices

    voice, _hubert, clips, _aux, _voices = enrolled
    hubert = StubHubert(gpu)
    with pytest.raises(OSError, match="3~10 seconds"):
        enroll_voices(voice, hubert, [clips[0], _clip(2.9, 32000, 60, 0.5)])
    with pytest.raises(OSError, match="3~10 seconds"):
        enroll_voices(voice, hubert, [_clip(10.1, 32000, 61, 0.5)])
    assert hubert.seen == []                                             # refused before any pass
    with pytest.raises(ValueError):
        enroll_voices(voice, hubert, clips, aux=[[]])


def test_clips16k_are_used_as_given(gpu, enrolled):
    from easevoice_trainer_amd.inference.semantic import prompt_semantics
    from easevoice_trainer_amd.inference.voice import enroll_voices

    voice, _hubert, clips, _aux, voices = enrolled
    given = [_clip(3.5, 16000, 70, 0.5), _clip(5.0, 16000, 71, 0.5)]
    hubert = StubHubert(gpu)
    got = enroll_voices(voice, hubert, clips[:2], clips16k=given)
    assert len(hubert.seen) == 1
    for seen, c in zip(hubert.seen[0], given):
        assert torch.equal(seen[:c.numel()].cpu(), c)
    want = prompt_semantics(StubHubert(gpu), voice.extract_latent, [c.to(gpu) for c in given])
    for v in range(2):
        assert torch.equal(got[v].prompt_semantic, want[v])
    # without aux clips a voice's style is its vector; clip 0's spectrogram does not depend on what it is batched with
    assert tuple(got[0].style.shape) == (1, 512) and got[0].frames == voices[0].frames

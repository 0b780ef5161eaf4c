"""GPU: the three entry points that take audio from the user -- audiokit/slicer.py::slice_batch, FeatureWriter.ssl_batch and
inference/voice.py::enroll_voices -- given WAV files of other rates, encodings and channel counts (tests/ingest_refs.py
writes them with struct).  A file gives what the array hip/audio.py::load_audio_batch makes of it gives; a 32 kHz PCM16 file
gives what train/dataset.py::read_wav_pcm16 of it gives, as before.  Clips are 3 .. 12 s with the planted silences of
tests/slicer_inputs.py where slicing is tested."""
import json
import os

import numpy as np
import pytest
import torch

import ingest_refs as R
import slicer_inputs as I

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PLAN = [(I.QUIET, 300), (I.LOUD, 4500), (I.QUIET, 800), (I.LOUD, 4400), (I.QUIET, 500)]        # 10.5 s, two clips
PLAN_B = [(I.LOUD, 4200), (I.QUIET, 1500), (I.LOUD, 4300)]                                      # 10 s, the long-silence branch


def _pcm(x, bits):
    return np.round(x.astype(np.float64) * (2 ** (bits - 1) - 1)).astype(np.int64)


def _stereo(left, seed):
    """[frames, 2]: the second channel is the first at another level plus a little noise of its own"""
    right = left * np.float32(0.5) + I.noise(len(left), seed) * np.float32(1e-3)
    return np.stack([left, right], axis=1)


def _file(tmp, name, fmt, samples, rate):
    path = str(tmp / name)
    samples = np.asarray(samples).reshape(len(samples), -1)
    R.wav_file(path, R.sample_bytes(samples, fmt), fmt, samples.shape[1], rate)
    return path


def _facts(result):
    ok, slices = result
    return ok, [(s.name, s.start, s.end, s.pcm.cpu().numpy().tobytes(), s.peak.cpu().numpy().tobytes()) for s in slices]


def test_slice_batch_files_of_other_rates_next_to_an_array(gpu, tmp_path):
    from easevoice_trainer_amd.audiokit import slicer as SL
    from easevoice_trainer_amd.hip import audio

    a = _file(tmp_path, "a.wav", R.S16, _pcm(_stereo(I.from_plan(PLAN, 48000, 21), 22), 16), 48000)
    b = _file(tmp_path, "b.wav", R.S24, _pcm(I.from_plan(PLAN_B, 44100, 23), 24), 44100)
    c = I.from_plan(PLAN, 32000, 24)
    names = ["dir/a.wav", "b.wav", "c.wav"]
    stats = {}
    got = SL.slice_batch(names, [a, c, b], stats=stats)
    assert stats["upload_s"] > 0 and stats["ingest_events"][0].elapsed_time(stats["ingest_events"][1]) >= 0
    pa = audio.load_audio_batch([a, b], 32000, gpu)
    assert pa.lengths == [len(c), (441 * 100) * 10 * 320 // 441]
    arrays = [pa.row(0).cpu().numpy(), c, pa.row(1).cpu().numpy()]
    want = SL.slice_batch(names, arrays)
    assert [_facts(g) for g in got] == [_facts(w) for w in want]
    assert [len(s) for _ok, s in got] == [2, 2, 2] and all(ok for ok, _s in got)
    for r in range(3):                                           # and every recording alone
        assert _facts(SL.slice_batch(names[r:r + 1], [[a, c, b][r]])[0]) == _facts(want[r])


def test_slice_batch_pcm16_files_at_the_slicers_rate_are_unchanged(gpu, tmp_path):
    from easevoice_trainer_amd.audiokit import slicer as SL
    from easevoice_trainer_amd.train.dataset import read_wav_pcm16

    x = I.from_plan(PLAN, 32000, 31)
    for k, samples in enumerate((_pcm(x, 16), _pcm(_stereo(x, 32), 16))):
        path = _file(tmp_path, f"take{k}.wav", R.S16, samples, 32000)
        got = SL.slice_batch([f"take{k}.wav"], [path], out_dir=str(tmp_path / f"file{k}"))
        want = SL.slice_batch([f"take{k}.wav"], [read_wav_pcm16(path, 32000)], out_dir=str(tmp_path / f"array{k}"))
        assert _facts(got[0]) == _facts(want[0]) and got[0][0] and len(got[0][1]) == 2
        written = sorted(os.listdir(tmp_path / f"array{k}" / "slices"))
        assert written == sorted(os.listdir(tmp_path / f"file{k}" / "slices")) == sorted(s.name for s in got[0][1])
        for name in written:
            assert (open(tmp_path / f"file{k}" / "slices" / name, "rb").read()
                    == open(tmp_path / f"array{k}" / "slices" / name, "rb").read()), name


def test_ssl_batch_takes_a_path(gpu, tmp_path):
    """the files written for a path are the files written for the array load_audio_batch makes of it; a name that has its
    feature file is skipped before its path is looked at"""
    from test_hubert_rows_gpu import _hub

    from easevoice_trainer_amd.feature_extractor.normalize import FeatureWriter
    from easevoice_trainer_amd.hip import audio

    hub = _hub(gpu, torch.float32)
    rs = np.random.RandomState(8)
    path = _file(tmp_path, "clip48.wav", R.S16, _pcm(_stereo((rs.rand(3 * 48000 + 7) - 0.5).astype(np.float32), 41), 16), 48000)
    clip = audio.load_audio_batch([path], 32000, gpu).row(0).cpu().numpy()
    other = (rs.rand(32000 + 11) - 0.5).astype(np.float32)
    assert len(clip) == (3 * 48000 + 7) * 2 // 3
    from_path, from_array = FeatureWriter(str(tmp_path / "p"), hub, None), FeatureWriter(str(tmp_path / "a"), hub, None)
    torch.save(torch.zeros(1), tmp_path / "p" / "4-cnhubert" / "have.wav.pt")
    assert from_path.ssl_batch(["o.wav", "have.wav", "x.wav"], [other, str(tmp_path / "no_such_file.wav"), path]) == [True] * 3
    assert from_array.ssl_batch(["o.wav", "x.wav"], [other, clip]) == [True] * 2
    for name in ("o.wav", "x.wav"):
        got, want = (torch.load(tmp_path / d / "4-cnhubert" / (name + ".pt")) for d in ("p", "a"))
        assert got.shape == want.shape and torch.equal(got, want), name
        assert open(tmp_path / "p" / "5-wav32k" / name, "rb").read() == open(tmp_path / "a" / "5-wav32k" / name, "rb").read()
    assert sorted(os.listdir(tmp_path / "p" / "5-wav32k")) == ["o.wav", "x.wav"]


@pytest.fixture(scope="module")
def voice(gpu):
    from util_fill import fill_module

    from easevoice_trainer_amd.inference.sovits import SoVITSVoice
    from easevoice_trainer_amd.module import models

    hps = json.load(open(os.path.join(ROOT, "configs", "s2.json")))
    net = models.SynthesizerTrn(1025, 32, n_speakers=300, **hps["model"])
    fill_module(net, 1)
    weight = {k: v.detach().clone() for k, v in net.state_dict().items() if "enc_q" not in k}
    return SoVITSVoice({"weight": weight, "config": hps, "info": "fixture"}, device=str(gpu), dtype=torch.bfloat16)


def test_enroll_voices_takes_paths(gpu, voice, tmp_path, monkeypatch):
    """a 48 kHz stereo file as the main clip (next to a voice given as an array, with an aux clip given as a 44.1 kHz file):
    the style of the ingested 32 kHz array; the prompt clip ingested from the file at 16 kHz in one step, inside the bound
    of the float64 resample of the file's decoded samples; a 2 s file is refused before any upload"""
    from test_enroll_voices_gpu import StubHubert, _clip

    from easevoice_trainer_amd.hip import audio
    from easevoice_trainer_amd.inference.semantic import PROMPT_TAIL
    from easevoice_trainer_amd.inference.voice import enroll_voices

    x = _pcm(_stereo(I.noise(4 * 48000 + 5, 51) * np.float32(0.6), 52), 16)
    path = _file(tmp_path, "voice48.wav", R.S16, x, 48000)
    aux_path = _file(tmp_path, "aux44.wav", R.S24, _pcm(I.noise(2 * 44100, 53) * np.float32(0.5), 24), 44100)
    second = _clip(3.5, 32000, 54, 0.8)
    hubert = StubHubert(gpu)
    got = enroll_voices(voice, hubert, [path, second], aux=[[aux_path], []])
    pa = audio.load_audio_batch([path, aux_path], 32000, gpu)
    arrays = [pa.row(0).cpu(), pa.row(1).cpu()]
    hubert_a = StubHubert(gpu)
    want = enroll_voices(voice, hubert_a, [arrays[0], second], aux=[[arrays[1]], []])
    for v in range(2):
        assert torch.equal(got[v].style, want[v].style) and got[v].frames == want[v].frames, v
    # the prompt clips: the file in one step, the array through 32 -> 16 kHz as before
    direct = audio.load_audio_batch([path], 16000, gpu).row(0)
    assert len(hubert.seen) == 1 and len(hubert.seen[0]) == 2 and direct.numel() == (4 * 48000 + 5) // 3
    seen = hubert.seen[0][0]
    assert seen.numel() == direct.numel() + PROMPT_TAIL and torch.equal(seen[:direct.numel()], direct)
    assert bool((seen[direct.numel():] == 0).all())
    assert torch.equal(hubert.seen[0][1], hubert_a.seen[0][1])
    assert not torch.equal(seen, hubert_a.seen[0][0][:seen.numel()])           # two steps are other samples
    wanted, bound = R.oracle(R.mono(x, R.S16), 1, 3)
    err = np.abs(direct.double().cpu().numpy() - wanted)
    worst = int(np.argmax(err - bound))
    print(f"prompt clip 48000 -> 16000: max err {err.max():.3e}, at the tightest place err {err[worst]:.3e} bound {bound[worst]:.3e}")
    assert (err <= bound).all()
    assert torch.equal(got[1].prompt_semantic, want[1].prompt_semantic)
    # the 3 .. 10 s rule on frames / rate from the header, before anything is uploaded
    short = _file(tmp_path, "short.wav", R.S16, _pcm(I.noise(2 * 48000, 55) * np.float32(0.5), 16), 48000)
    long = _file(tmp_path, "long.wav", R.U8, np.full((10 * 8000 + 1, 1), 128), 8000)
    monkeypatch.setattr(audio, "upload_raw", lambda *a, **k: pytest.fail("uploaded"))
    fresh = StubHubert(gpu)
    for bad in (short, long):
        with pytest.raises(OSError, match="3~10 seconds"):
            enroll_voices(voice, fresh, [path, bad])
    assert fresh.seen == []

"""No GPU: the host logic of the batched `token` step -- inference/semantic.py::write_semantic_tsv_batch / prompt_semantics and
feature_extractor/normalize.py::FeatureWriter.ssl_batch(tokens=True) / write_semantic -- with stand-ins of the two models
that have the real signatures and run in plain torch on the CPU.  The stand-in quantiser is a fixed function of a frame
pair, so `extract_latent` ([B, 768, T] -> [B, 1, T // 2]) and `extract_latent_rows` ((hs [B, Tmax, 768], frames) -> B views
of one packed buffer) agree by construction and every difference the tests find is the host code's."""
import os

import numpy as np
import pytest
import torch

from easevoice_trainer_amd.feature_extractor.normalize import FeatureWriter
from easevoice_trainer_amd.inference import semantic as S


class StandInVoice:
    """code of a frame pair = a hash of its two leading channels; `calls` records (B, Tmax, frames) of every rows call"""
    device = "cpu"

    def __init__(self):
        self.calls, self.single = [], 0

    @staticmethod
    def _codes(pairs):                                   # [n, 2, 768] -> [n]
        return ((pairs[:, 0, 0] * 37.0 + pairs[:, 1, 1] * 11.0).abs().floor().long()) % 1024

    def extract_latent(self, ssl):                       # [B, 768, T] -> [B, 1, T // 2]
        self.single += 1
        B, C, T = ssl.shape
        x = ssl.transpose(1, 2)[:, : T // 2 * 2].reshape(B * (T // 2), 2, C)
        return self._codes(x).view(B, 1, T // 2)

    def extract_latent_rows(self, hs, frames):
        assert hs.dim() == 3 and hs.size(2) == 768 and len(frames) == hs.size(0) and hs.dtype == torch.float32
        self.calls.append((hs.size(0), hs.size(1), list(frames)))
        packed = torch.cat([self._codes(hs[b, : t // 2 * 2].reshape(t // 2, 2, 768)) for b, t in enumerate(frames)])
        return list(torch.split(packed, [t // 2 for t in frames]))


class StandInHubert:
    """frames as CN-HuBERT counts them; frame t of a clip = a ramp scaled by the mean magnitude of its 320 samples.  A clip
    whose first sample is exactly 0.125 comes out non-finite (ssl_batch must refuse it)."""
    device = "cpu"

    def __init__(self):
        self.batches = 0

    def last_hidden_state_batch(self, wavs):
        self.batches += 1
        rows, lens = wavs
        frames = [(int(n) - 400) // 320 + 1 for n in lens]
        hs = torch.zeros(len(lens), max(frames), 768)
        ramp = torch.linspace(0.5, 1.5, 768)
        for b, t in enumerate(frames):
            level = rows[b, : t * 320].view(t, 320).abs().mean(1, keepdim=True)
            hs[b, :t] = (1.0 + level) * ramp * (1.0 + torch.arange(t)[:, None] * 0.37)
            if float(rows[b, 0]) == 0.125:
                hs[b, 0, 0] = float("inf")
        return hs, frames

    def batch(self, wavs):
        hs, frames = self.last_hidden_state_batch(wavs)
        return [hs[b:b + 1, :t].transpose(1, 2).clone() for b, t in enumerate(frames)]


class CpuFrontWriter(FeatureWriter):
    """FeatureWriter with the device half in front of the model (_front_rows: two launches and a resampler) replaced by
    its definition on the host; `uploads` counts how often it ran"""
    uploads = 0

    def _front_rows(self, clips):
        self.uploads += 1
        peaks = [float(np.abs(c).max()) for c in clips]
        wav16 = [(np.nan_to_num(c) * 100).astype(np.int16) for c in clips]
        lens = [len(c) // 2 for c in clips]
        rows = torch.zeros(len(clips), max(lens))
        for b, c in enumerate(clips):
            rows[b, : lens[b]] = torch.from_numpy(np.ascontiguousarray(c[: 2 * lens[b]: 2]))
        return peaks, wav16, rows, lens


def _feature_dir(tmp_path, frames):
    d = tmp_path / "4-cnhubert"
    d.mkdir()
    g = torch.Generator().manual_seed(3)
    names = []
    for i, t in enumerate(frames):
        names.append(f"item{i}.wav")
        f = torch.randn(1, t, 768, generator=g) * 3
        # as CNHubert saves them: a transposed view of [1, T, 768] (torch.save keeps the strides); every third one C-contiguous
        torch.save(f.transpose(1, 2).contiguous() if i % 3 == 2 else f.transpose(1, 2), d / (names[-1] + ".pt"))
    return str(d), names


@pytest.mark.parametrize("group", [1, 4, 16])
def test_batch_file_equals_per_item_file(tmp_path, group):
    hubert_dir, names = _feature_dir(tmp_path, [101, 2, 57, 1, 300, 64, 33])
    asked = ["nofile.wav"] + names[::-1] + ["other.wav"]                    # order kept, names without a file skipped
    v = StandInVoice()
    n1 = S.write_semantic_tsv(v.extract_latent, asked, hubert_dir, str(tmp_path / "one.tsv"))
    n2 = S.write_semantic_tsv_batch(v.extract_latent_rows, asked, hubert_dir, str(tmp_path / "rows.tsv"), group=group,
                                    device="cpu")
    assert n1 == n2 == 7
    one = open(tmp_path / "one.tsv", "rb").read()
    assert one == open(tmp_path / "rows.tsv", "rb").read()
    lines = one.decode("utf8").split("\n")
    assert [ln.split("\t")[0] for ln in lines[1:-1]] == names[::-1] and lines[-1] == ""
    assert lines[4] == "item3.wav\t"                                        # one frame: no code, an empty field as before
    assert len(v.calls) == -(-7 // group)                                   # one call per group, padded to its longest item
    fr = [33, 64, 300, 1, 57, 2, 101]
    assert v.calls == [(len(fr[i:i + group]), max(fr[i:i + group]), fr[i:i + group]) for i in range(0, 7, group)]
    with pytest.raises(ValueError):
        S.write_semantic_tsv_batch(v.extract_latent_rows, asked, hubert_dir, str(tmp_path / "x.tsv"), group=0, device="cpu")


def test_empty_list_writes_the_header(tmp_path):
    hubert_dir, _names = _feature_dir(tmp_path, [])
    v = StandInVoice()
    assert S.write_semantic_tsv_batch(v.extract_latent_rows, ["a"], hubert_dir, str(tmp_path / "r.tsv"), device="cpu") == 0
    S.write_semantic_tsv(v.extract_latent, ["a"], hubert_dir, str(tmp_path / "o.tsv"))
    assert open(tmp_path / "r.tsv", "rb").read() == open(tmp_path / "o.tsv", "rb").read() == b"item_name\tsemantic_audio\n"
    assert v.calls == []


def test_codes_to_host_takes_views_and_plain_lists():
    base = torch.arange(10)
    rows = list(torch.split(base, [3, 0, 7]))
    assert S.codes_to_host(rows) == [[0, 1, 2], [], list(range(3, 10))]
    assert S.codes_to_host([base[5:], base[:5]]) == [list(range(5, 10)), list(range(5))]        # not in packed order
    assert S.codes_to_host([torch.tensor([4, 5]), torch.tensor([6])]) == [[4, 5], [6]] and S.codes_to_host([]) == []


def _clips():
    rs = np.random.RandomState(2)
    clips = [(rs.rand(n).astype(np.float32) - 0.5) for n in (3200, 4801, 6400, 4000, 3600)]
    clips[1][7] = np.nan                  # non-finite peak: refused
    clips[2] *= 6.0                       # peak above 2.2: skipped, nothing written
    clips[3][0] = 0.125                   # the stand-in HuBERT returns non-finite features for it
    return ["n0.wav", "n1.wav", "n2.wav", "n3.wav", "n4.wav"], clips


def test_ssl_batch_tokens_then_write_semantic(tmp_path):
    names, clips = _clips()
    plain = CpuFrontWriter(str(tmp_path / "plain"), StandInHubert(), None)
    hub, voice = StandInHubert(), StandInVoice()
    want_done = [True, False, True, False, True]
    assert plain.ssl_batch(names, clips) == want_done
    fw = CpuFrontWriter(str(tmp_path / "tok"), hub, None, voice=voice)
    assert fw.ssl_batch(names, clips, tokens=True) == want_done                    # the return value is unchanged
    assert len(voice.calls) == 1 and voice.calls[0][0] == 3                        # n0, n3, n4 went through in one call
    for sub in ("4-cnhubert", "5-wav32k"):                                         # and so are the files
        a, b = sorted(os.listdir(tmp_path / "plain" / sub)), sorted(os.listdir(tmp_path / "tok" / sub))
        assert a == b and len(a) == 2
    for n in ("n0.wav", "n4.wav"):
        f = torch.load(tmp_path / "tok" / "4-cnhubert" / (n + ".pt"))
        assert torch.equal(f, torch.load(tmp_path / "plain" / "4-cnhubert" / (n + ".pt")))
        assert fw._codes[n] == voice.extract_latent(f)[0, 0].tolist()              # the codes of the file
    assert sorted(fw._codes) == ["n0.wav", "n4.wav"]                               # skipped / refused items: no codes
    calls = len(voice.calls)
    assert fw.write_semantic(names) == 2
    assert len(voice.calls) == calls                                               # kept codes: no file is tokenised
    S.write_semantic_tsv(voice.extract_latent, names, str(tmp_path / "tok" / "4-cnhubert"), str(tmp_path / "want.tsv"))
    assert open(tmp_path / "tok" / "6-name2semantic.tsv", "rb").read() == open(tmp_path / "want.tsv", "rb").read()


def test_write_semantic_mixes_kept_codes_and_files(tmp_path):
    names, clips = _clips()
    voice, hub = StandInVoice(), StandInHubert()
    fw = CpuFrontWriter(str(tmp_path), hub, None, voice=voice)
    torch.save(torch.randn(1, 768, 41, generator=torch.Generator().manual_seed(5)), tmp_path / "4-cnhubert" / "old.wav.pt")
    torch.save(torch.randn(1, 768, 12, generator=torch.Generator().manual_seed(6)), tmp_path / "4-cnhubert" / "n4.wav.pt")
    done = fw.ssl_batch(names[:1] + names[4:], clips[:1] + clips[4:], tokens=True)   # n4 has a file already: skipped
    assert done == [True, True] and sorted(fw._codes) == ["n0.wav"]
    order = ["old.wav", "gone.wav", "n4.wav", "n0.wav", "old.wav"]
    assert fw.write_semantic(order, group=1) == 4
    assert [c[2] for c in voice.calls[1:]] == [[41], [12]]                           # the two files, a group each, once each
    S.write_semantic_tsv(voice.extract_latent, order, str(tmp_path / "4-cnhubert"), str(tmp_path / "want.tsv"))
    assert open(tmp_path / "6-name2semantic.tsv", "rb").read() == open(tmp_path / "want.tsv", "rb").read()
    # close() is what it was
    fw.close()
    assert open(tmp_path / "2-name2text.txt").read() == "\n"


def test_tokens_without_voice_raises_before_any_upload(tmp_path):
    names, clips = _clips()
    fw = CpuFrontWriter(str(tmp_path / "a"), StandInHubert(), None)
    with pytest.raises(ValueError):
        fw.ssl_batch(names, clips, tokens=True)
    only_call = lambda wav: torch.zeros(1, 768, 3)                                  # a hubert without last_hidden_state_batch
    fw2 = CpuFrontWriter(str(tmp_path / "b"), only_call, None, voice=StandInVoice())
    with pytest.raises(ValueError):
        fw2.ssl_batch(names, clips, tokens=True)
    assert fw.uploads == 0 and fw2.uploads == 0 and os.listdir(tmp_path / "a" / "4-cnhubert") == []
    with pytest.raises(ValueError):                                                 # files to tokenise and no voice
        torch.save(torch.zeros(1, 768, 4), tmp_path / "a" / "4-cnhubert" / "x.pt")
        fw.write_semantic(["x"])


def test_prompt_semantics_with_and_without_rows():
    class PromptHubert:
        def last_hidden_state_batch(self, clips):
            rows = torch.zeros(len(clips), max(c.numel() for c in clips))
            for b, c in enumerate(clips):
                rows[b, : c.numel()] = c
            return StandInHubert().last_hidden_state_batch((rows, [c.numel() for c in clips]))

    g = torch.Generator().manual_seed(4)
    wavs = [torch.rand(n, generator=g) - 0.5 for n in (48000, 70001, 160000)]
    voice = StandInVoice()
    old = S.prompt_semantics(PromptHubert(), voice.extract_latent, wavs)
    assert voice.single == 1 and voice.calls == []
    new = S.prompt_semantics(PromptHubert(), voice.extract_latent, wavs, extract_latent_rows=voice.extract_latent_rows)
    assert voice.single == 1 and len(voice.calls) == 1                              # the padded path is not taken
    assert len(old) == len(new) == 3
    for a, b in zip(old, new):
        assert a.dtype == b.dtype == torch.int64 and a.dim() == 1 and torch.equal(a, b)
    assert new[0]._base is None                                                     # copies, not views of the packed buffer
    with pytest.raises(OSError):
        S.prompt_semantics(PromptHubert(), voice.extract_latent, [wavs[0][:100]], extract_latent_rows=voice.extract_latent_rows)
    bad = lambda hs, frames: [torch.zeros(1, dtype=torch.long)] * len(frames)
    with pytest.raises(ValueError):
        S.prompt_semantics(PromptHubert(), voice.extract_latent, wavs, extract_latent_rows=bad)

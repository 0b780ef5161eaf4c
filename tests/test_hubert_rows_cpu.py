"""Host side of CN-HuBERT on ragged batches (no GPU): the frame arithmetic of HubertModel.forward_rows, the skip / return
logic of FeatureWriter.ssl_batch and the padding / cut of inference.semantic.prompt_semantics with stub models, and the C ABI
of the two new entry points in both builds of the library."""
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def test_forward_rows_frame_arithmetic():
    from easevoice_trainer_amd.feature_extractor.cnhubert import CONV_KERNEL, CONV_STRIDE, MIN_SAMPLES, HubertModel
    from easevoice_trainer_amd.hip import feat

    for n in range(400, 421):
        per_layer = HubertModel.layer_frames(n)
        assert len(per_layer) == 7 and per_layer[-1] == HubertModel.frames(n) == 1
        assert per_layer[0] == feat.front_frames(n) == (n - 10) // 5 + 1
        for i in range(1, 7):
            assert per_layer[i] == (per_layer[i - 1] - CONV_KERNEL[i]) // CONV_STRIDE[i] + 1
    assert HubertModel.layer_frames(16000)[-1] == HubertModel.frames(16000) == 49
    assert HubertModel.frames(719) == 1 and HubertModel.frames(720) == 2
    assert MIN_SAMPLES == 400 and HubertModel.frames(399) == 0 and feat.front_frames(9) == 0 and feat.front_frames(10) == 1
    assert HubertModel.check_clip_lengths([400, 9000], 9000) == [400, 9000]
    with pytest.raises(ValueError):
        HubertModel.check_clip_lengths([9000, 399], 9000)
    with pytest.raises(ValueError):
        HubertModel.check_clip_lengths([9001], 9000)
    # forward_rows refuses before it touches a device
    model = HubertModel(layers=1)
    with pytest.raises(ValueError):
        model.forward_rows(torch.zeros(2, 1000), [1000, 399])
    with pytest.raises(ValueError):
        model.forward_rows(torch.zeros(2, 1000), [1000])


class _StubHubert:
    """stands for CNHubert behind FeatureWriter / prompt_semantics: records what it is given"""
    device = torch.device("cpu")

    def __init__(self, poison=()):
        self.calls, self.poison = [], set(poison)

    def _frames(self, n):
        from easevoice_trainer_amd.feature_extractor.cnhubert import HubertModel

        return HubertModel.frames(n)

    def batch(self, rows_lens):
        rows, lens = rows_lens
        self.calls.append((rows.clone(), list(lens)))
        out = []
        for b, n in enumerate(lens):
            t = torch.full((1, 768, self._frames(n)), float(rows[b, :n].abs().max()))
            if n in self.poison:
                t[0, 3, 0] = float("inf")
            out.append(t)
        return out

    def last_hidden_state_batch(self, clips):
        self.calls.append([c.clone() for c in clips])
        lens = [self._frames(c.numel()) for c in clips]
        return torch.zeros(len(clips), max(lens), 768), lens


def _host_front_rows(clips):
    """FeatureWriter._front_rows on the host, from the single-clip functions"""
    from easevoice_trainer_amd.feature_extractor.normalize import MAXX, ALPHA, resample_half

    peaks, wav16, rows = [], [], []
    for c in clips:
        peak = np.abs(c).max()
        with np.errstate(all="ignore"):
            a32 = (c / peak * (MAXX * ALPHA * 32768)) + ((1 - ALPHA) * 32768) * c
            a32b = (c / peak * (MAXX * ALPHA * 1145.14)) + ((1 - ALPHA) * 1145.14) * c
            wav16.append(np.nan_to_num(np.clip(a32, -32768, 32767)).astype("int16"))
        peaks.append(float(peak))
        rows.append(resample_half(a32b.astype(np.float32)))
    lens = [len(r) for r in rows]
    out = torch.zeros(len(rows), max(lens))
    for b, r in enumerate(rows):
        out[b, :lens[b]] = torch.from_numpy(r)
    return peaks, wav16, out, lens


def test_ssl_batch_skip_and_return_logic(tmp_path):
    from easevoice_trainer_amd.feature_extractor.normalize import FeatureWriter, rescale_clip

    rs = np.random.RandomState(2)
    mk = lambda n: (rs.rand(n) - 0.5).astype(np.float32)  # noqa: E731
    hub = _StubHubert(poison={1100})
    w = FeatureWriter(str(tmp_path), hub, None)
    uploads = []
    w._front_rows = lambda clips: (uploads.append([len(c) for c in clips]), _host_front_rows(clips))[1]
    torch.save(torch.zeros(1), tmp_path / "4-cnhubert" / "have.wav.pt")
    # every name exists: nothing is uploaded, the model is not run
    assert w.ssl_batch(["have.wav"], [mk(2000)]) == [True] and not uploads and not hub.calls
    loud, bad, ok, poisoned = mk(2400) * 8, mk(2600), mk(3000), mk(2200)       # 2200 -> 1100 samples at 16 kHz: poisoned
    assert np.abs(loud).max() > 2.2
    bad[7] = np.nan
    names = ["have.wav", "loud.wav", "nan.wav", "inf.wav", "ok.wav"]
    assert w.ssl_batch(names, [mk(2000), loud, bad, poisoned, ok]) == [True, True, False, False, True]
    assert uploads == [[2400, 2600, 2200, 3000]]                               # the existing name was dropped before upload
    assert len(hub.calls) == 1 and hub.calls[0][1] == [1100, 1500]             # one pass, without the loud and the NaN clip
    assert hub.calls[0][0].shape == (2, 1500) and not hub.calls[0][0][0, 1100:].any()
    assert sorted(os.listdir(tmp_path / "4-cnhubert")) == ["have.wav.pt", "ok.wav.pt"]
    assert os.listdir(tmp_path / "5-wav32k") == ["ok.wav"]
    from scipy.io import wavfile

    rate, data = wavfile.read(tmp_path / "5-wav32k" / "ok.wav")
    assert rate == 32000 and np.array_equal(data, rescale_clip(ok)[0])
    assert torch.load(tmp_path / "4-cnhubert" / "ok.wav.pt").shape == (1, 768, 4)
    assert w.ssl_batch(names[-1:], [ok]) == [True] and len(hub.calls) == 1       # now it exists
    with pytest.raises(ValueError):
        w.ssl_batch(["x", "y"], [ok])


def test_prompt_semantics_padding_and_cut():
    from easevoice_trainer_amd.inference.semantic import PROMPT_TAIL, prompt_semantics

    hub = _StubHubert()
    seen = []

    def extract(ssl):
        seen.append(tuple(ssl.shape))
        b, _, t = ssl.shape
        return (torch.arange(t // 2)[None, None] + 1000 * torch.arange(b)[:, None, None]).long()

    clips = [torch.ones(48000), torch.ones(65600), torch.ones(160000)]
    codes = prompt_semantics(hub, extract, clips)
    assert PROMPT_TAIL == int(0.3 * 32000) == 9600
    got = hub.calls[0]
    for c, g in zip(clips, got):
        assert g.numel() == c.numel() + 9600 and bool((g[:c.numel()] == 1).all()) and not g[c.numel():].any()
    frames = [hub._frames(c.numel() + 9600) for c in clips]
    assert frames == [179, 234, 529] and seen == [(3, 768, 529)]
    assert [c.numel() for c in codes] == [f // 2 for f in frames]
    for b, c in enumerate(codes):
        assert c.dim() == 1 and c.tolist() == [1000 * b + i for i in range(frames[b] // 2)]
    for n in (32000, 47999, 160001):
        with pytest.raises(OSError):
            prompt_semantics(hub, extract, [clips[0], torch.ones(n)])
    assert prompt_semantics(hub, extract, []) == []


def test_libraries_export_the_rows_entry_points():
    """both builds export evt_hubert_front_rows / evt_clip_rescale_rows, and the bindings pass as many arguments as
    include/evt.h declares (the existing ABI test's way: the header is the list)"""
    from easevoice_trainer_amd.hip import lib as L

    hdr = open(os.path.join(HERE, "..", "include", "evt.h")).read()
    declared = {}
    for name in ("evt_hubert_front_rows", "evt_clip_rescale_rows", "evt_hubert_front_ws_floats"):
        m = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in evt.h"
        declared[name] = len(m.group(1).split(","))
    assert declared == {"evt_hubert_front_rows": 13, "evt_clip_rescale_rows": 8, "evt_hubert_front_ws_floats": 2}
    for half in (torch.bfloat16, torch.float16):
        L.set_half(half)
        lib = L.lib()
        for name, count in declared.items():
            assert hasattr(lib, name), f"{name} is not exported by the {half} build"
            assert len(getattr(lib, name).argtypes) == count, f"{name} of the {half} build"
        assert lib.evt_hubert_front_ws_floats(3, 9000) == 3 * 512 * (29 + 2)        # host arithmetic, no launch
        # NULL pointers are refused before anything is launched
        assert lib.evt_hubert_front_rows(L.DT_F32, None, None, 1, 100, None, None, None, 1e-5, None, None, 0, None) == 22
        assert lib.evt_clip_rescale_rows(None, None, 1, 100, None, None, None, None) == 22
    L.set_half(torch.bfloat16)

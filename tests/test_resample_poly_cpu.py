"""CPU: the host side of the packed-audio output (hip/audio.py, inference/pipeline.py) -- the resampler's prototype filter and
phase table against feature_extractor/normalize.py (whose resample_half the operator is at the ratio 1/2), output lengths,
and the way out_rate / out_format travel through synthesize_stream / synthesize_pcm: on the emulated s1 session of
tests/test_pipeline_batch_cpu.py with a stub voice and a recording stand-in for the one launch."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import resample_oracle as O
from cpu_emu_stream_force import cpu_emulation_stream_force
from test_pipeline_batch_cpu import POLL, STOPS, STOPS2, StubVoice, _inputs, _model


def test_taps_at_one_half_are_the_half_band_taps():
    from easevoice_trainer_amd.feature_extractor.normalize import _half_band_taps
    from easevoice_trainer_amd.hip.audio import poly_taps

    g = poly_taps(1, 2)
    assert g.dtype == np.float64 and g.shape == (255,)
    assert np.abs(g[127:] - _half_band_taps()).max() <= 1e-15
    assert np.array_equal(g, g[::-1])
    # the tests' own statement of the formula agrees with the package's at every ratio in use
    for rate in O.RATES:
        up, down = O.ratio(rate)
        if up == down:
            continue
        want, h = O.taps(up, down)
        got = poly_taps(up, down)
        assert got.shape == (2 * h - 1,) and np.abs(got - want).max() <= 1e-15, rate


@pytest.mark.parametrize("rate", [r for r in O.RATES if r != O.IN_RATE] + [500])
def test_phase_table_regroups_the_taps_exactly(rate):
    """every g[k] appears exactly once, as T[k mod up][R - (k - k mod up) / up]; everything else -- the corners no tap
    reaches and the padding to a multiple of 4 -- is zero"""
    from easevoice_trainer_amd.hip.audio import phase_rows, poly_taps, table_shape

    up, down = O.ratio(rate)
    g = poly_taps(up, down)
    h = (len(g) + 1) // 2
    r, j_pad = table_shape(up, down)
    t = phase_rows(up, down)
    assert t.dtype == np.float64 and t.shape == (up, j_pad) and j_pad % 4 == 0 and 2 * r + 1 <= j_pad <= 2 * r + 4
    assert r == -(-64 * max(up, down) // up)
    k = np.arange(-(h - 1), h)
    p = k % up
    j = r - (k - p) // up
    assert j.min() >= 0 and j.max() <= 2 * r
    assert len(set(zip(p.tolist(), j.tolist()))) == len(k), "no two taps share a cell"
    assert np.array_equal(t[p, j], g)
    rest = t.copy()
    rest[p, j] = 0.0
    assert not rest.any(), "cells without a tap are zero"


def test_definition_at_one_half_is_resample_half():
    """the float64 oracle of the definition against normalize.resample_half (which rounds its result to float32) on 700
    samples of seeded noise: within 2^-24 |want| + 1e-12"""
    from easevoice_trainer_amd.feature_extractor.normalize import resample_half

    x = np.random.default_rng(5).standard_normal(700)
    want = resample_half(x).astype(np.float64)
    got, _a, _j = O.resample(x, 1, 2)
    assert got.shape == want.shape == (350,)
    err = np.abs(got - want)
    print("max |oracle - resample_half| =", err.max())
    assert (err <= 2.0 ** -24 * np.abs(want) + 1e-12).all()


def test_phase_form_equals_the_definition():
    """sum_j T[p][j] x[q - R + j] in float64 is the direct sum, at a ratio up (3/2), down (1/4) and 441/320"""
    from easevoice_trainer_amd.hip.audio import phase_rows, table_shape

    x = np.random.default_rng(6).standard_normal(97)
    for up, down in ((3, 2), (1, 4), (441, 320)):
        want, a, _j = O.resample(x, up, down)
        r, j_pad = table_shape(up, down)
        t = phase_rows(up, down)
        xp = np.concatenate([np.zeros(r), x, np.zeros(j_pad + r + 1)])
        got = np.array([t[(m * down) % up] @ xp[(m * down) // up:(m * down) // up + j_pad] for m in range(len(want))])
        assert np.abs(got - want).max() <= 1e-15 * a.max() * j_pad, (up, down)


def test_output_lengths_and_ratios():
    from easevoice_trainer_amd.hip import audio
    from easevoice_trainer_amd.hip.lib import EvtError

    assert list(audio.RATES) == O.RATES
    want = {8000: (1, 4), 16000: (1, 2), 22050: (441, 640), 24000: (3, 4), 32000: (1, 1), 44100: (441, 320), 48000: (3, 2)}
    for rate in O.RATES:
        up, down = audio.rate_ratio(32000, rate)
        assert (up, down) == want[rate]
        for n in (0, 1, 2, 37, 641):
            assert audio.out_len(n, up, down) == (n * up) // down
            if n:
                assert len(O.resample(np.ones(n), up, down)[0]) == (n * up) // down
    with pytest.raises(EvtError, match="1024"):
        audio.rate_ratio(32000, 44101)
    with pytest.raises(EvtError, match="1024"):
        audio.rate_ratio(32000, 11025)            # 441 / 1280
    with pytest.raises(EvtError):
        audio.rate_ratio(32000, 0)


# ---------------------------------------------------------------------------------------------------------------------
# the keywords' way through the pipeline

RATE, INTERVAL = 16000, 0.3


def _fake_pack(record):
    """stands in for hip.audio.resample_pack: records the call; a row's "audio" is its values as int16 / float32"""
    from easevoice_trainer_amd.hip.audio import FORMATS, PackedAudio

    def pack(x, lens, mul, in_rate, out_rate, out_format, order=None, interval=0.0, **kw):
        x = x.reshape(1, -1) if x.dim() == 1 else x.reshape(x.size(0), -1)
        record.append(dict(nseq=x.size(0), lens=list(lens), mul=mul, in_rate=in_rate, out_rate=out_rate,
                           out_format=out_format, order=order, interval=interval))
        rows = [x[b, :lens[b] * mul].to(FORMATS[out_format][1]) for b in range(x.size(0))]
        offs = np.concatenate([[0], np.cumsum([r.numel() for r in rows])]).tolist()
        return PackedAudio(torch.cat(rows), offs[:-1], [r.numel() for r in rows], out_rate, 0)

    return pack


class PackingVoice(StubVoice):
    """StubVoice whose decode_batch answers out_rate / out_format as SynthesizerTrn.decode_batch does: with a PackedAudio"""

    def __init__(self, pack):
        super().__init__()
        self.pack = pack

    def decode_batch(self, codes, code_lens, text, text_lens, refer, **kw):
        out = {k: kw[k] for k in ("out_rate", "out_format") if k in kw}
        wavs = super().decode_batch(codes, code_lens, text, text_lens, refer, **kw)
        if not out:
            return wavs
        x = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True)
        return self.pack(x, [w.numel() for w in wavs], 1, 32000, out.get("out_rate", 32000), out.get("out_format", "float32"))


@pytest.fixture(scope="module")
def runs():
    from easevoice_trainer_amd.auto_reg.t2s_infer import StreamControl
    from easevoice_trainer_amd.hip import audio
    from easevoice_trainer_amd.inference.pipeline import synthesize_pcm, synthesize_stream

    d = _inputs()
    # fragment 0 finishes last (step 10) and fragment 7 at the first poll, so that the stream's order is not the input order
    q = d["q"]
    q[STOPS[0], 0, 1024], q[STOPS[7], 7, 1024] = 1.0, 1.0
    q[10, 0, 1024], q[2, 7, 1024] = 1e-30, 1e-30
    out = {"inputs": d}
    saved = audio.resample_pack
    try:
        with cpu_emulation_stream_force():
            m = _model()
            t2s = SimpleNamespace(model=m, device="cpu", early_stop_num=14)
            kw = dict(top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35, slots=8,
                      sample_kwargs=dict(noise=d["q"], poll=POLL))
            args = lambda voice: (t2s, voice, d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], [])
            for name, fn, extra in (
                    ("plain", synthesize_stream, dict(s2_batch=4)),
                    ("rate", synthesize_stream, dict(s2_batch=4, out_rate=48000)),
                    ("format", synthesize_stream, dict(s2_batch=4, out_format="int16")),
                    ("single", synthesize_stream, dict(out_rate=RATE, out_format="int16")),
                    ("pcm", synthesize_pcm, dict(s2_batch=4, out_rate=RATE, fragment_interval=INTERVAL)),
                    ("pcm_ctl", synthesize_pcm, dict(s2_batch=4, fragment_interval=0.01, control="4,6"))):
                if extra.get("control"):
                    ctl = StreamControl()
                    ctl.preempt(6)
                    ctl.cancel(4)
                    extra = dict(extra, control=ctl)
                record = []
                audio.resample_pack = _fake_pack(record)
                voice = PackingVoice(audio.resample_pack)
                got = fn(*args(voice), **kw, **extra)
                out[name] = (got if fn is synthesize_pcm else list(got), voice.calls, record)
            # two takes per fragment outside the groups (s2_batch = 1): the chosen take is decoded alone
            q2 = torch.empty(16, 8, 1025).exponential_(1, generator=torch.Generator().manual_seed(78))
            for r, s in enumerate(STOPS2):
                q2[s, r, 1024] = 1e-30
            record = []
            audio.resample_pack = _fake_pack(record)
            voice = PackingVoice(audio.resample_pack)
            got = list(synthesize_stream(*args(voice), **dict(kw, slots=16, sample_kwargs=dict(
                noise=torch.stack([d["q"], q2], 2).contiguous(), poll=POLL)), candidates=2, choose=lambda i, outs: i % 2,
                out_format="int16"))
            out["cand"] = (got, voice.calls, record)
    finally:
        audio.resample_pack = saved
    return out


def test_keywords_reach_decode_batch_only_when_set(runs):
    for name, want in (("plain", {}), ("rate", {"out_rate": 48000}), ("format", {"out_format": "int16"})):
        got, calls, record = runs[name]
        assert [k for k, *_ in calls] == ["decode_batch", "decode_batch", "decode", "decode"], name
        for kind, _sems, _phones, _speed, kw in calls:
            assert kw == (want if kind == "decode_batch" else {}), (name, kind, kw)
    assert runs["plain"][2] == [], "without the keywords nothing is packed"
    assert all(w.dtype == torch.float32 for _r, w in runs["plain"][0])
    assert all(w.dtype == torch.int16 for _r, w in runs["format"][0])


def test_a_lone_fragment_is_decode_then_one_row_pack(runs):
    # the two lonely fragments of the grouped run: decode, then resample_pack with nseq = 1 at the keywords that were set
    for name, rate, fmt in (("rate", 48000, "float32"), ("format", 32000, "int16")):
        got, calls, record = runs[name]
        lone = [c for c in record if c["nseq"] == 1]
        assert len(record) == 4 and len(lone) == 2, name
        for c in record:
            assert (c["in_rate"], c["out_rate"], c["out_format"], c["mul"], c["interval"]) == (32000, rate, fmt, 1, 0.0), c
    # s2_batch = 1: eight decode calls, eight one-row packs, the same audio as the groups give
    got, calls, record = runs["single"]
    assert [k for k, *_ in calls] == ["decode"] * 8 and all(kw == {} for *_x, kw in calls)
    assert [c["nseq"] for c in record] == [1] * 8
    assert all((c["out_rate"], c["out_format"]) == (RATE, "int16") for c in record)
    plain = dict(runs["plain"][0])
    for r, w in got:
        assert w.dtype == torch.int16 and torch.equal(w, plain[r].to(torch.int16)), r
        assert record[[q for q, _w in got].index(r)]["lens"] == [plain[r].numel()]


def test_candidates_path_is_decode_then_one_row_pack(runs):
    got, calls, record = runs["cand"]
    assert sorted(r for r, _w in got) == list(range(8)) and all(w.dtype == torch.int16 for _r, w in got)
    assert [k for k, *_ in calls] == ["decode"] * 8 and all(kw == {} for *_x, kw in calls)
    assert [(c["nseq"], c["out_rate"], c["out_format"]) for c in record] == [(1, 32000, "int16")] * 8
    for (r, w), (_k, sems, *_rest) in zip(got, calls):
        assert torch.equal(w, sems[0].to(torch.int16)), r


def test_pcm_is_the_references_postprocess(runs):
    """TTS.audio_postprocess (tts.py:878-908) on the fragments the stream yields: input order, int(rate * interval) zeros
    behind every fragment, int16; one tensor on the host"""
    (rate, pcm), calls, record = runs["pcm"]
    plain = dict(runs["plain"][0])
    assert [r for r, _w in runs["plain"][0]] != sorted(plain), "the stream's order is not the input order here"
    zero = np.zeros(int(RATE * INTERVAL), dtype=np.int16)
    want = np.concatenate([a for r in range(8) for a in (plain[r].numpy().astype(np.int16), zero)])
    assert rate == RATE and pcm.dtype == torch.int16 and pcm.device.type == "cpu" and pcm.dim() == 1
    assert zero.size == 4800 and np.array_equal(pcm.numpy(), want)
    assert all((c["out_rate"], c["out_format"]) == (RATE, "int16") for c in record) and len(record) == 4
    for kind, *_x, kw in calls:
        assert kw == ({"out_rate": RATE, "out_format": "int16"} if kind == "decode_batch" else {})


def test_pcm_skips_cancelled_fragments(runs):
    (rate, pcm), calls, record = runs["pcm_ctl"]
    plain = dict(runs["plain"][0])
    assert rate == 32000, "out_rate None is the model's rate"
    zero = np.zeros(int(32000 * 0.01), dtype=np.int16)
    want = np.concatenate([a for r in (0, 1, 2, 3, 5, 7) for a in (plain[r].numpy().astype(np.int16), zero)])
    assert np.array_equal(pcm.numpy(), want)

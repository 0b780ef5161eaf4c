"""CPU: synthesize_stream(fragment_style=[...]) -- a voice per fragment through the s2 decoder.  The emulated s1 session,
the inputs (six fragments finish at the first poll, one alone at the second, one alone at the third) and the recording stub
voice are tests/test_pipeline_batch_cpu.py's; the stub here also records what it is handed as `refer` and `style`.

With fragment_style every group's decode_batch call gets refer = None and the stacked styles of exactly its fragments, in
order; a lone fragment gets decode(refer=None, style=its own); cancelled and preempted fragments pass through; a list of
the wrong length is a ValueError; without the keyword the recorded calls are the parent's."""
from types import SimpleNamespace

import pytest
import torch

from cpu_emu_stream_force import cpu_emulation_stream_force
from test_pipeline_batch_cpu import POLL, StubVoice, _inputs, _model

GIN = 16


class VoiceStub(StubVoice):
    """StubVoice that also keeps (refer, style) of every call, in `handed`"""

    def __init__(self):
        super().__init__()
        self.handed = []

    def decode(self, sem, phones, refer, speed=1.0, style=None, **kw):
        self.handed.append((refer, style))
        return super().decode(sem, phones, refer, speed=speed, **kw)

    def decode_batch(self, codes, code_lens, text, text_lens, refer, style=None, **kw):
        self.handed.append((refer, style))
        if style is None:
            return super().decode_batch(codes, code_lens, text, text_lens, refer, **kw)
        # the parent's stub insists on a list of one shared reference: with styles there is none
        assert refer is None
        got = super().decode_batch(codes, code_lens, text, text_lens, [None] * codes.size(1), **kw)
        return got


def _styles():
    g = torch.Generator().manual_seed(5)
    return [torch.randn(1, GIN, generator=g) for _ in range(8)]


@pytest.fixture(scope="module")
def runs():
    from easevoice_trainer_amd.auto_reg.t2s_infer import StreamControl
    from easevoice_trainer_amd.inference.pipeline import synthesize_stream

    d, styles, out = _inputs(), _styles(), {}
    with cpu_emulation_stream_force():
        m = _model()
        t2s = SimpleNamespace(model=m, device="cpu", early_stop_num=14)
        kw = dict(top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35, slots=8,
                  sample_kwargs=dict(noise=d["q"], poll=POLL))

        def go(name, voice, refer_specs, **extra):
            got = list(synthesize_stream(t2s, voice, d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], refer_specs,
                                         **kw, **extra))
            out[name] = (got, voice.calls, getattr(voice, "handed", None))

        shared = [torch.zeros(1, 4, 3)]
        go("parent_stub", StubVoice(), shared, s2_batch=4)                 # the parent's stub: refuses an unknown keyword
        go("plain", VoiceStub(), shared, s2_batch=4)
        go("plain_one", VoiceStub(), shared)
        go("styled", VoiceStub(), [], s2_batch=4, fragment_style=styles)
        go("styled_one", VoiceStub(), [], fragment_style=styles)
        go("enrolled", VoiceStub(), [], s2_batch=4,
           fragment_style=[SimpleNamespace(style=s, prompt_semantic=None, frames=0) for s in styles])
        ctl = StreamControl()
        ctl.preempt(6)
        ctl.cancel(4)
        go("control", VoiceStub(), [], s2_batch=4, fragment_style=styles, control=ctl)
    out["styles"], out["inputs"] = styles, d
    return out


def _rows_of(runs, name):
    """per call the fragments it decoded: the stub's waveform is the fragment's tokens, and all eight differ"""
    waves = {r: w for r, w in runs["plain"][0]}
    groups = []
    for _k, sems, *_ in runs[name][1]:
        g = []
        for s in sems:
            hits = [r for r, w in waves.items() if w.numel() == s.numel() and torch.equal(w, s.float())]
            assert len(hits) == 1
            g.append(hits[0])
        groups.append(g)
    return groups


def test_groups_get_the_stacked_styles_of_their_fragments(runs):
    got, calls, handed = runs["styled"]
    styles, groups = runs["styles"], _rows_of(runs, "styled")
    assert [k for k, *_ in calls] == ["decode_batch", "decode_batch", "decode", "decode"]
    assert [len(g) for g in groups] == [4, 2, 1, 1] and sorted(r for g in groups for r in g) == list(range(8))
    for g, (refer, style) in zip(groups, handed):
        assert refer is None
        assert tuple(style.shape) == (len(g), GIN)
        assert torch.equal(style, torch.cat([styles[r] for r in g], 0)), g
    # the same fragments in the same order with the same waveforms as without the keyword
    assert [r for r, _w in got] == [r for r, _w in runs["plain"][0]]
    assert all(torch.equal(a, b) for (_r, a), (_q, b) in zip(got, runs["plain"][0]))
    assert groups == _rows_of(runs, "plain")
    assert all("style" not in kw and "refer" not in kw for *_x, kw in calls)


def test_enrolled_voices_are_taken_by_their_style(runs):
    for (_r1, s1), (_r2, s2) in zip(runs["enrolled"][2], runs["styled"][2]):
        assert _r1 is None and torch.equal(s1, s2)


def test_a_lone_fragment_gets_decode_with_its_style(runs):
    _got, calls, handed = runs["styled"]
    groups = _rows_of(runs, "styled")
    for g, (k, *_), (refer, style) in zip(groups, calls, handed):
        if len(g) == 1:
            assert k == "decode" and refer is None and torch.equal(style, runs["styles"][g[0]])
    # s2_batch = 1: eight decode calls, each with its own fragment's style
    got, calls, handed = runs["styled_one"]
    assert len(calls) == 8 and all(k == "decode" for k, *_ in calls)
    for (r, _w), (refer, style) in zip(got, handed):
        assert refer is None and tuple(style.shape) == (1, GIN) and torch.equal(style, runs["styles"][r])


def test_cancelled_and_preempted_pass_through(runs):
    got, calls, handed = runs["control"]
    res = dict(got)
    assert sorted(res) == list(range(8)) and res[4] is None and res[6] is None
    groups = _rows_of(runs, "control")
    assert sorted(r for g in groups for r in g) == [0, 1, 2, 3, 5, 7] and [len(g) for g in groups] == [4, 1, 1]
    for g, (refer, style) in zip(groups, handed):
        assert refer is None and torch.equal(style, torch.cat([runs["styles"][r] for r in g], 0))


def test_without_the_keyword_the_calls_are_the_parents(runs):
    """the parent's stub (no `style` parameter, refer asserted to be a list of one shared object) goes through unchanged, and
    the recording stub sees no style and the shared reference"""
    got_p, calls_p, _ = runs["parent_stub"]
    got, calls, handed = runs["plain"]
    assert [r for r, _w in got] == [r for r, _w in got_p]
    assert len(calls) == len(calls_p)
    for (k, sems, phones, speed, kw), (kp, sems_p, phones_p, speed_p, kw_p) in zip(calls, calls_p):
        assert k == kp and speed == speed_p and kw == kw_p == {}
        assert all(torch.equal(a, b) for a, b in zip(sems, sems_p)) and all(torch.equal(a, b) for a, b in zip(phones, phones_p))
    for (k, *_), (refer, style) in zip(calls, handed):
        assert style is None and isinstance(refer, list)
        if k == "decode_batch":
            assert all(r is refer[0] for r in refer) and isinstance(refer[0], list) and len(refer[0]) == 1
    assert all(style is None and len(refer) == 1 for refer, style in runs["plain_one"][2])


def test_wrong_length_raises(runs):
    from easevoice_trainer_amd.inference.pipeline import synthesize_pcm, synthesize_stream

    d = runs["inputs"]
    t2s = SimpleNamespace(model=None, device="cpu", early_stop_num=14)
    args = (t2s, VoiceStub(), d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], [])
    with pytest.raises(ValueError, match="fragment_style"):
        list(synthesize_stream(*args, fragment_style=runs["styles"][:7]))
    with pytest.raises(ValueError, match="fragment_style"):
        synthesize_pcm(*args, fragment_style=runs["styles"][:7])

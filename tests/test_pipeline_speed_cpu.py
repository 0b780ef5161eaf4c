"""CPU: synthesize_stream(fragment_speed=[...]) -- one speed per fragment.  With s2_batch > 1 the groups of one poll stay
batched and decode_batch gets the group's speeds (only when one of them is not 1); decoded alone, a fragment gets its own
speed through decode.  The session is the emulated one of tests/test_pipeline_batch_cpu.py (tests/cpu_emu_stream_force.py:
eight fragments, six finish at the first poll, one alone at the second, one alone at the third); a stub voice records
its calls."""
import os
from types import SimpleNamespace

import pytest
import torch
import yaml

from cpu_emu_stream_force import cpu_emulation_stream_force
from util_fill import fill_module

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

STOPS = [3, 2, 3, 2, 3, 2, 6, 10]      # step at which fragment r draws EOS
POLL = 4
NPROMPT = 12
MIXED = [0.8, 1.0, 1.25, 1.0, 1.0, 1.0, 1.5, 1.0]


def _model():
    from easevoice_trainer_amd.auto_reg.t2s_model import Text2SemanticDecoder

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "gpt.yaml")))
    m = Text2SemanticDecoder(cfg)
    fill_module(m, 3)
    m.eval()
    return m


def _inputs(seed=77):
    g = torch.Generator().manual_seed(seed)
    lens = [13, 9, 11, 10, 12, 9, 14, 10]
    ids = [torch.randint(0, 732, (n,), generator=g) for n in lens]
    bert = [torch.randn(1024, n, generator=g) for n in lens]
    q = torch.empty(16, len(lens), 1025).exponential_(1, generator=g)
    for r, s in enumerate(STOPS):
        q[s, r, 1024] = 1e-30
    return dict(all_ids=ids, bert=bert, batch_phones=[i[4:] for i in ids], q=q,
                prompt=torch.randint(0, 1024, (1, NPROMPT), generator=g))


class StubVoice:
    """records every s2 call as (kind, token rows, speed as passed -- None: no keyword); a waveform is the tokens as floats"""

    def __init__(self):
        self.calls = []
        self.model = self

    def decode(self, sem, phones, refer, speed=1.0, **kw):
        assert sem.dim() == 3 and sem.size(0) == 1 and sem.size(1) == 1 and kw == {}
        self.calls.append(("decode", [sem[0, 0].clone()], speed))
        return sem.float()

    def decode_batch(self, codes, code_lens, text, text_lens, refer, speed=None, **kw):
        B = codes.size(1)
        assert codes.dim() == 3 and codes.size(0) == 1 and len(code_lens) == B == len(text_lens) and kw == {}
        sems = [codes[0, b, :code_lens[b]].clone() for b in range(B)]
        self.calls.append(("decode_batch", sems, speed))
        return [s.float() for s in sems]


@pytest.fixture(scope="module")
def runs():
    """one emulated session per mode, each with its own stub voice: name -> (yielded, calls)"""
    from easevoice_trainer_amd.inference.pipeline import synthesize_stream

    d = _inputs()
    out = {"inputs": d}
    with cpu_emulation_stream_force():
        m = _model()
        t2s = SimpleNamespace(model=m, device="cpu", early_stop_num=14)
        kw = dict(top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35, slots=8,
                  sample_kwargs=dict(noise=d["q"], poll=POLL))

        def go(name, **extra):
            voice = StubVoice()
            args = (t2s, voice, d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], [])
            out[name] = (list(synthesize_stream(*args, **kw, **extra)), voice.calls)

        go("four", s2_batch=4)
        go("four_125", s2_batch=4, fragment_speed=[1.25] * 8)
        go("four_mixed", s2_batch=4, fragment_speed=MIXED)
        go("four_ones", s2_batch=4, fragment_speed=[1.0] * 8)
        go("one_mixed", s2_batch=1, fragment_speed=MIXED)
        go("default_mixed", fragment_speed=MIXED)
        errors = {}
        for name, extra in (("both", dict(s2_batch=4, speed_factor=1.25, fragment_speed=[1.25] * 8)),
                            ("both_single", dict(speed_factor=1.25, fragment_speed=[1.0] * 8)),
                            ("short", dict(s2_batch=4, fragment_speed=[1.25] * 7)),
                            ("long", dict(fragment_speed=[1.25] * 9))):
            voice = StubVoice()
            with pytest.raises(ValueError) as e:
                list(synthesize_stream(t2s, voice, d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], [], **kw, **extra))
            errors[name] = (str(e.value), voice.calls)
        out["errors"] = errors
    return out


def _fragment_of(runs, sem):
    """the fragment whose tokens `sem` is (the stub's waveform = the tokens; all eight differ)"""
    hits = [r for r, w in runs["four"][0] if w.numel() == sem.numel() and torch.equal(w, sem.float())]
    assert len(hits) == 1, hits
    return hits[0]


def _groups(runs, name):
    return [[_fragment_of(runs, s) for s in sems] for _k, sems, _v in runs[name][1]]


def test_batched_at_one_speed_per_fragment(runs):
    got, calls = runs["four_125"]
    got1, calls1 = runs["four"]
    assert [(k, len(sems)) for k, sems, _v in calls1] == [("decode_batch", 4), ("decode_batch", 2), ("decode", 1), ("decode", 1)]
    assert all(v is None for k, _s, v in calls1 if k == "decode_batch") and all(v == 1.0 for k, _s, v in calls1 if k == "decode")
    # same order, same groups, same calls as at speed 1
    assert [r for r, _w in got] == [r for r, _w in got1] and all(torch.equal(a, b) for (_r, a), (_q, b) in zip(got, got1))
    assert _groups(runs, "four_125") == _groups(runs, "four")
    assert [k for k, *_ in calls] == [k for k, *_ in calls1]
    for kind, sems, v in calls:
        if kind == "decode_batch":
            assert v == [1.25] * len(sems)
        else:
            assert v == 1.25                           # a fragment that finishes alone: decode at its own speed


def test_mixed_speeds_reach_their_rows(runs):
    got, calls = runs["four_mixed"]
    assert [r for r, _w in got] == [r for r, _w in runs["four"][0]]
    groups = _groups(runs, "four_mixed")
    assert groups == _groups(runs, "four")
    seen_batch = 0
    for g, (kind, _sems, v) in zip(groups, calls):
        if kind == "decode":
            assert v == MIXED[g[0]]
        elif any(MIXED[r] != 1.0 for r in g):
            assert v == [MIXED[r] for r in g]
            seen_batch += 1
        else:
            assert v is None                           # a group of speed-1 fragments: the call of today
    assert seen_batch >= 1
    assert sorted(r for g in groups for r in g) == list(range(8))


def test_all_ones_makes_the_calls_without_the_keyword(runs):
    got, calls = runs["four_ones"]
    assert [(k, len(s), v) for k, s, v in calls] == [(k, len(s), v) for k, s, v in runs["four"][1]]
    assert all(v is None for k, _s, v in calls if k == "decode_batch")
    assert all(torch.equal(a, b) for (_r, a), (_q, b) in zip(got, runs["four"][0]))


@pytest.mark.parametrize("name", ["one_mixed", "default_mixed"])
def test_single_decodes_carry_each_fragments_speed(runs, name):
    got, calls = runs[name]
    assert [r for r, _w in got] == [r for r, _w in runs["four"][0]]
    assert len(calls) == 8 and all(k == "decode" for k, *_ in calls)
    for (r, w), (_k, sems, v) in zip(got, calls):
        assert torch.equal(sems[0].float(), w) and v == MIXED[r], r


def test_candidates_path_decodes_alone_at_the_fragments_speed(runs):
    """candidates > 1 without s2 groups: the chosen take goes through decode(speed=fragment_speed[r])"""
    from easevoice_trainer_amd.inference.pipeline import synthesize_stream

    d = runs["inputs"]
    g2 = torch.Generator().manual_seed(78)
    q2 = torch.empty(16, 8, 1025).exponential_(1, generator=g2)
    for r, s in enumerate([2, 3, 2, 3, 2, 3, 5, 9]):
        q2[s, r, 1024] = 1e-30
    with cpu_emulation_stream_force():
        m = _model()
        t2s = SimpleNamespace(model=m, device="cpu", early_stop_num=14)
        voice = StubVoice()
        got = list(synthesize_stream(t2s, voice, d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], [], top_k=1100,
                                     top_p=1, temperature=1.0, repetition_penalty=1.35, slots=16,
                                     sample_kwargs=dict(noise=torch.stack([d["q"], q2], 2).contiguous(), poll=POLL),
                                     candidates=2, choose=lambda i, outs: 0, fragment_speed=MIXED))
    assert sorted(r for r, _w in got) == list(range(8)) and len(voice.calls) == 8
    for (r, _w), (k, _sems, v) in zip(got, voice.calls):
        assert k == "decode" and v == MIXED[r], r


def test_errors_come_before_any_decode(runs):
    e = runs["errors"]
    assert "speed_factor" in e["both"][0] and "speed_factor" in e["both_single"][0]
    assert "7 entries for 8" in e["short"][0] and "9 entries for 8" in e["long"][0]
    assert all(calls == [] for _msg, calls in e.values())

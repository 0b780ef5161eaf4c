"""CPU: synthesize_stream(s2_batch=k) -- fragments that the refilled s1 session (auto_reg/t2s_infer.py, launches emulated
on the session's buffers: tests/cpu_emu_stream_force.py) completes at the SAME poll go through the s2 decoder in groups of
at most k, one decode_batch call per group; a stub voice records its calls.  The polls are read back from the session's
own record (stream_stats["events"]: the step count of every finish), never from the grouping under test.

Eight fragments; EOS is planted through the noise table (top_k covers the vocabulary) at the steps STOPS, and the session
polls every 4 steps: six fragments finish at the first poll (steps 1..4), one alone at the second, one alone at the third."""
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
STOPS2 = [2, 3, 2, 3, 2, 3, 5, 9]     # the same for the second take of test_candidates_go_through_the_batch
POLL = 4
NPROMPT = 12


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
    """records every s2 call; a waveform is the fragment's tokens as floats"""

    def __init__(self):
        self.calls = []
        self.model = self

    def decode(self, sem, phones, refer, speed=1.0, **kw):
        assert sem.dim() == 3 and sem.size(0) == 1 and sem.size(1) == 1 and phones.dim() == 2 and phones.size(0) == 1
        self.calls.append(("decode", [sem[0, 0].clone()], [phones[0].clone()], float(speed), kw))
        return sem.float()

    def decode_batch(self, codes, code_lens, text, text_lens, refer, **kw):
        B = codes.size(1)
        assert codes.dim() == 3 and codes.size(0) == 1 and text.shape[0] == B and len(code_lens) == B == len(text_lens)
        assert codes.size(2) == max(code_lens) and text.size(1) == max(text_lens)
        assert isinstance(refer, list) and len(refer) == B and all(r is refer[0] for r in refer)
        sems = [codes[0, b, :code_lens[b]].clone() for b in range(B)]
        self.calls.append(("decode_batch", sems, [text[b, :text_lens[b]].clone() for b in range(B)], 1.0, kw))
        return [s.float() for s in sems]


@pytest.fixture(scope="module")
def runs():
    """one emulated session per mode, each with its own stub voice: (yielded, calls, finish step per fragment)"""
    from easevoice_trainer_amd.auto_reg.t2s_infer import StreamControl
    from easevoice_trainer_amd.inference.pipeline import synthesize_stream

    d = _inputs()
    out = {}
    with cpu_emulation_stream_force():
        m = _model()
        t2s = SimpleNamespace(model=m, device="cpu", early_stop_num=14)
        kw = dict(top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35, slots=8,
                  sample_kwargs=dict(noise=d["q"], poll=POLL))

        def go(name, **extra):
            voice = StubVoice()
            args = (t2s, voice, d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], [])
            got = list(synthesize_stream(*args, **kw, **extra))
            ev = m._infer().stream_stats["events"]
            out[name] = (got, voice.calls, {r: s for kind, s, r, _slot in ev if kind == "finish"}, list(ev))

        go("parent")                                       # the keyword left out
        go("one", s2_batch=1)
        go("four", s2_batch=4)
        go("speed", s2_batch=4, speed_factor=1.25)
        ctl = StreamControl()
        ctl.preempt(6)          # still running at the first poll: handed out with partial tokens -> (6, None)
        ctl.cancel(4)
        go("control", s2_batch=4, control=ctl)
        slow = dict(kw, slots=3)
        ctl2 = StreamControl()
        ctl2.cancel(5)          # still waiting for a slot when its turn comes: no prompt pass, (5, None)
        voice = StubVoice()
        got = list(synthesize_stream(t2s, voice, d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], [],
                                     **slow, s2_batch=4, control=ctl2))
        ev = m._infer().stream_stats["events"]
        out["refill"] = (got, voice.calls, {r: s for kind, s, r, _slot in ev if kind == "finish"}, list(ev))
        # two takes per fragment; the second take's EOS steps keep every fragment in the poll of its first take
        g2 = torch.Generator().manual_seed(78)
        q2 = torch.empty(16, 8, 1025).exponential_(1, generator=g2)
        for r, s in enumerate(STOPS2):
            q2[s, r, 1024] = 1e-30
        asked = []

        def choose(i, outs):
            asked.append((i, outs))
            return i % 2

        voice = StubVoice()
        got = list(synthesize_stream(t2s, voice, d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], [],
                                     **dict(kw, slots=16, sample_kwargs=dict(noise=torch.stack([d["q"], q2], 2).contiguous(),
                                                                             poll=POLL)),
                                     s2_batch=4, candidates=2, choose=choose))
        out["cand"] = (got, voice.calls, asked, list(m._infer().stream_stats["events"]))
    out["inputs"] = d
    return out


def _fragment_of(runs, sem):
    """the fragment whose tokens `sem` is (the stub's waveform = the tokens; all eight differ)"""
    hits = [r for r, w in runs["parent"][0] if w is not None and w.numel() == sem.numel() and torch.equal(w, sem.float())]
    assert len(hits) == 1, hits
    return hits[0]


def test_session_polls_as_planned(runs):
    """the scenario the other tests rely on: six finishes at step 4, one at 8, one at 12"""
    _got, _calls, fin, _ev = runs["parent"]
    assert fin == {0: 4, 1: 4, 2: 4, 3: 4, 4: 4, 5: 4, 6: 8, 7: 12}


def test_s2_batch_1_issues_the_parents_calls(runs):
    got_p, calls_p, _f, _e = runs["parent"]
    got_1, calls_1, _f1, _e1 = runs["one"]
    assert [r for r, _w in got_p] == [r for r, _w in got_1]
    assert all(torch.equal(a, b) for (_r, a), (_q, b) in zip(got_p, got_1))
    assert len(calls_p) == len(calls_1) == 8
    d = runs["inputs"]
    for (r, w), cp, c1 in zip(got_p, calls_p, calls_1):
        for kind, sems, phones, speed, kw in (cp, c1):
            assert kind == "decode" and speed == 1.0 and kw == {}
            assert torch.equal(sems[0].float(), w) and torch.equal(phones[0], d["batch_phones"][r])


def test_groups_are_one_poll_and_at_most_four(runs):
    got, calls, fin, _ev = runs["four"]
    groups = [[_fragment_of(runs, s) for s in sems] for _k, sems, _p, _s, _kw in calls]
    # six fragments of the first poll: 4 + 2; the two lonely ones: one decode each
    assert [len(g) for g in groups] == [4, 2, 1, 1]
    assert [k for k, *_ in calls] == ["decode_batch", "decode_batch", "decode", "decode"]
    for g in groups:
        assert len({fin[r] for r in g}) == 1, (g, fin)
        assert len(g) <= 4
    assert sorted(r for g in groups for r in g) == list(range(8))
    d = runs["inputs"]
    for g, (_k, _sems, phones, _s, _kw) in zip(groups, calls):
        for r, ph in zip(g, phones):
            assert torch.equal(ph, d["batch_phones"][r])


def test_arrival_order_and_indices(runs):
    got, calls, fin, _ev = runs["four"]
    got_p = runs["parent"][0]
    assert [r for r, _w in got] == [r for r, _w in got_p]            # the order the session delivered them in
    waves = dict(got_p)
    for r, w in got:
        assert torch.equal(w, waves[r]), r
    # a group's rows are in arrival order too
    order = [r for r, _w in got]
    flat = [_fragment_of(runs, s) for _k, sems, _p, _s, _kw in calls for s in sems]
    assert flat == order


def test_speed_falls_back_to_single_decodes(runs):
    got, calls, _fin, _ev = runs["speed"]
    assert [r for r, _w in got] == [r for r, _w in runs["parent"][0]]
    assert len(calls) == 8 and all(k == "decode" and s == 1.25 for k, _a, _b, s, _kw in calls)


def test_cancelled_and_preempted_pass_through(runs):
    got, calls, fin, ev = runs["control"]
    res = dict(got)
    assert sorted(res) == list(range(8)) and len(got) == 8
    assert res[6] is None and res[4] is None
    assert all(res[r] is not None for r in (0, 1, 2, 3, 5, 7))
    kinds = {r: k for k, _s, r, _slot in ev if k != "admit"}
    assert kinds[6] == "preempt" and kinds[4] == "cancel"
    decoded = sorted(_fragment_of(runs, s) for _k, sems, _p, _s, _kw in calls for s in sems)
    assert decoded == [0, 1, 2, 3, 5, 7]                               # no s2 call for 4 and 6
    assert [len(sems) for _k, sems, *_ in calls] == [4, 1, 1]          # five live ones at the first poll: 4 + 1; then 7
    waves = dict(runs["parent"][0])
    for r, w in got:
        assert w is None or torch.equal(w, waves[r])
    # arrival order = the order of the session's own record
    assert [r for r, _w in got] == [r for k, _s, r, _slot in ev if k != "admit"]


def test_refilled_session_groups_by_poll(runs):
    """3 slots for 8 fragments: slots are refilled, a fragment cancelled while it waits comes out between two polls"""
    got, calls, fin, ev = runs["refill"]
    res = dict(got)
    assert sorted(res) == list(range(8)) and res[5] is None
    assert [(k, slot) for k, _s, r, slot in ev if r == 5] == [("cancel", None)]
    waves = dict(runs["parent"][0])
    for r, w in got:
        assert w is None or torch.equal(w, waves[r]), r
    groups = [[_fragment_of(runs, s) for s in sems] for _k, sems, _p, _s, _kw in calls]
    assert sorted(r for g in groups for r in g) == [0, 1, 2, 3, 4, 6, 7]
    by_poll = {}
    for r, s in fin.items():
        by_poll.setdefault(s, []).append(r)
    assert sorted(sorted(g) for g in groups) == sorted(sorted(v) for v in by_poll.values())   # <= 3 per poll here
    for g, (k, *_rest) in zip(groups, calls):
        assert k == ("decode" if len(g) == 1 else "decode_batch")
    # events are in delivery order
    assert [r for r, _w in got] == [r for k, _s, r, _slot in ev if k != "admit"]


def test_candidates_go_through_the_batch(runs):
    """candidates=2 with s2_batch=4: choose is asked once per fragment when both takes are in, and the chosen takes of one
    poll are decoded together"""
    got, calls, asked, ev = runs["cand"]
    assert sorted(i for i, _o in asked) == list(range(8)) and sorted(r for r, _w in got) == list(range(8))
    chosen = {i: outs[i % 2] for i, outs in asked}
    for r, w in got:
        t = chosen[r]
        assert torch.equal(w, t.y[-t.idx:].float()), r
    assert [r for r, _w in got] == [i for i, _o in asked]
    assert [(k, len(sems)) for k, sems, *_ in calls] == [("decode_batch", 4), ("decode_batch", 2), ("decode", 1), ("decode", 1)]
    flat = [s for _k, sems, *_ in calls for s in sems]
    for (r, _w), s in zip(got, flat):
        t = chosen[r]
        assert torch.equal(s, t.y[-t.idx:])
    fin = {}
    for k, s, r, _slot in ev:
        if k == "finish":
            fin.setdefault(r, set()).add(s)
    assert all(len(v) == 1 for v in fin.values())          # both takes of a fragment at one poll, as planned


def test_s2_batch_must_be_positive():
    from easevoice_trainer_amd.inference.pipeline import synthesize_stream

    t2s = SimpleNamespace(model=None, device="cpu", early_stop_num=20)
    with pytest.raises(ValueError, match="s2_batch"):
        list(synthesize_stream(t2s, None, [], [], [], torch.zeros(1, 4, dtype=torch.long), [], s2_batch=0))

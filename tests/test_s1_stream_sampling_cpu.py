"""CPU: per-request sampling parameters and cancellation in a refilled s1 decode session (auto_reg/t2s_infer.py
decode_stream / StreamControl), launches emulated on the session's buffers with the sampler reading each row's parameters
from the session's table (tests/cpu_emu_stream_rows.py).  Reference: tests/golden/s1_mixed_sampling.pt, the reference's
infer_panel_batch_infer on 12 texts once per parameter set; request r of a mixed session is set r % 4's row r."""
import os
import sys

import pytest
import torch
import yaml

from cpu_emu_stream_rows import cpu_emulation_stream_rows
from util_fill import fill_module

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))


def _model():
    from easevoice_trainer_amd.auto_reg.t2s_model import Text2SemanticDecoder

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "gpt.yaml")))
    m = Text2SemanticDecoder(cfg)
    fill_module(m, 3)
    m.eval()
    return m


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(HERE, "golden", "s1_mixed_sampling.pt"), weights_only=False)


@pytest.fixture(scope="module")
def inputs(gold):
    from make_golden_s1_rows import rows_inputs

    return rows_inputs(gold["R"])


def _expect(gold, r):
    s = gold["sets"][r % 4]
    return s["y"][r].long(), s["idx"][r]


def _requests(d, gold, rows, form=dict):
    sets = [s["args"] for s in gold["sets"]]
    return [(d["x"][r], d["bert"][r], d["prompts"][r], form(sets[r % 4])) for r in rows]


def test_mixed_sets_match_reference_tokens(gold, inputs):
    """twelve requests with parameter sets r % 4 through 5 slots of one session: request for request the reference's
    tokens and index under that request's own set; the session-wide values are a fifth set no request keeps"""
    R, d = gold["R"], inputs
    with cpu_emulation_stream_rows():
        m = _model()
        out = {r: (y, i) for r, y, i in m.decode_stream(_requests(d, gold, range(R)), slots=5, noise=d["q"], top_k=3,
                                                        top_p=0.5, temperature=2.0, repetition_penalty=1.1,
                                                        early_stop_num=gold["early_stop_num"])}
        st = m._infer().stream_stats
    assert sorted(out) == list(range(R)) and st["admissions"] >= 3 and sum(st["admitted"]) == R
    for r in range(R):
        y, idx = _expect(gold, r)
        assert out[r][1] == idx, (r, out[r][1], idx)
        assert torch.equal(out[r][0].long(), y), r
    # the fixture separates the sets: the same text decodes differently under another set
    assert not torch.equal(gold["sets"][0]["y"][1].long(), gold["sets"][1]["y"][1].long())


def test_list_form_of_the_refill_call(gold, inputs):
    """infer_panel_batch_infer_refill with a sequence of length R for each of the five parameters: the same result"""
    R, d = gold["R"], inputs
    sets = [s["args"] for s in gold["sets"]]
    per = {k: [sets[r % 4][k] for r in range(R)] for k in ("top_k", "top_p", "temperature", "repetition_penalty")}
    per["early_stop_num"] = [gold["early_stop_num"]] * R
    with cpu_emulation_stream_rows():
        m = _model()
        ys, idxs = m.infer_panel_batch_infer_refill(d["x"], d["x_lens"], d["prompts"], d["bert"], slots=5, noise=d["q"],
                                                    **per)
        from easevoice_trainer_amd.hip.lib import EvtError
        with pytest.raises(EvtError, match="top_p"):
            m.infer_panel_batch_infer_refill(d["x"], d["x_lens"], d["prompts"], d["bert"], slots=5, noise=d["q"],
                                             **dict(per, top_p=[1.0] * (R - 1)))
    for r in range(R):
        y, idx = _expect(gold, r)
        assert idxs[r] == idx and torch.equal(ys[r].long(), y), r


@pytest.mark.parametrize("bad,what", [(dict(top_q=0.5), "top_q"), (dict(repetition_penalty=0), "repetition_penalty"),
                                      (dict(temperature=float("nan")), "temperature")],
                         ids=["unknown_key", "penalty_zero", "nan_temperature"])
@pytest.mark.parametrize("lazy", [False, True], ids=["list", "generator"])
def test_bad_request_is_refused_before_its_admission(gold, inputs, bad, what, lazy):
    """an unknown key, repetition_penalty = 0 and a NaN temperature raise EvtError naming request 2: for a list before
    anything is launched at all, for a generator when the request is drawn (requests 0 and 1 are running by then)"""
    from easevoice_trainer_amd.hip.lib import EvtError

    d = inputs
    reqs = [(d["x"][r], d["bert"][r], d["prompts"][r], bad if r == 2 else 3) for r in range(4)]
    kw = dict(slots=2, noise=d["q"], top_k=1100, top_p=1, early_stop_num=3, poll=1)
    with cpu_emulation_stream_rows():
        m = _model()
        if not lazy:
            with pytest.raises(EvtError, match=f"request 2: .*{what}"):
                m.decode_stream(reqs, **kw)
            assert getattr(m._infer(), "stream_stats", None) is None
        else:
            g = m.decode_stream(iter(reqs), max_text_len=24, max_prompt_len=12, **kw)
            first = next(g)
            assert first[0] in (0, 1)
            with pytest.raises(EvtError, match=f"request 2: .*{what}"):
                list(g)
            st = m._infer().stream_stats
            assert [r for kind, _s, r, _slot in st["events"] if kind == "admit"] == [0, 1]


def test_session_wide_values_are_validated(inputs):
    from easevoice_trainer_amd.hip.lib import EvtError

    d = inputs
    reqs = [(d["x"][0], d["bert"][0], d["prompts"][0])]
    with cpu_emulation_stream_rows():
        m = _model()
        with pytest.raises(EvtError, match="repetition_penalty"):
            m.decode_stream(reqs, noise=d["q"], repetition_penalty=-1.0)
        with pytest.raises(EvtError, match="top_p"):
            m.decode_stream(reqs, noise=d["q"], top_p=float("inf"))


def cancel_scenario(m, d, gold, dev="cpu", on_cancel=None):
    """8 requests (set A, the fixture's rows 4..11 reordered so that lives differ) through 3 slots, poll 1.  After the
    first item has been yielded the request in slot 0 and a request still waiting are cancelled.  Returns (items of the
    run with cancellation, its events, items of the run without, the two cancelled request indices)."""
    from easevoice_trainer_amd.auto_reg.t2s_infer import StreamControl

    rows = [0, 11, 10, 4, 5, 9, 6, 7]          # request 0 runs to the early stop; 1 and 2 stop at steps 1 and 2
    a = dict(gold["sets"][0]["args"], early_stop_num=gold["early_stop_num"], slots=3, poll=1)
    q = d["q"][:, rows].contiguous().to(dev)
    reqs = [(d["x"][r].to(dev), d["bert"][r].to(dev), d["prompts"][r].to(dev)) for r in rows]
    plain = list(m.decode_stream(reqs, noise=q, **a))
    ev_plain = list(m._infer().stream_stats["events"])
    ctl = StreamControl()
    got = []
    for item in m.decode_stream(reqs, noise=q, control=ctl, **a):
        got.append(item)
        if len(got) == 1:
            ctl.cancel(0)                       # admitted first: slot 0, still running (it lives 13 steps)
            ctl.cancel(6)                       # still in the queue
            ctl.cancel(99)                      # unknown: ignored
            ctl.cancel(item[0])                 # already delivered: ignored
        if item[1] is None and on_cancel is not None:
            on_cancel(item[0])
    return got, list(m._infer().stream_stats["events"]), plain, ev_plain, (0, 6)


def check_cancel(got, events, plain, ev_plain, cancelled):
    ref = {r: (y, i) for r, y, i in plain}
    assert sorted(r for r, _y, _i in got) == list(range(8))
    for r, y, i in got:
        if r in cancelled:
            assert y is None and i is None, r
        else:
            assert i == ref[r][1] and torch.equal(y, ref[r][0]), r
    assert all(kind != "cancel" for kind, *_ in ev_plain)
    cancels = {r: (step, slot) for kind, step, r, slot in events if kind == "cancel"}
    assert sorted(cancels) == list(cancelled)
    step0, slot0 = cancels[0]
    assert slot0 == 0 and cancels[6][1] is None
    assert not any(kind == "admit" and r == 6 for kind, _s, r, _slot in events)        # no prompt pass for it
    # the freed slot is taken by the admission of that same poll
    assert any(kind == "admit" and slot == 0 and step == step0 for kind, step, _r, slot in events[1:]), events
    # the cancel arrived after the first hand-out and acted at the poll after it
    first_finish = min(step for kind, step, _r, _slot in events if kind == "finish")
    assert step0 == first_finish + 1
    # without the cancel, request 0 keeps slot 0 for 12 replays
    assert [s for k, s, r, _ in ev_plain if k == "finish" and r == 0][0] >= 12


def test_cancel_running_and_waiting(gold, inputs):
    """StreamControl.cancel on 8 requests through 3 slots: see cancel_scenario / check_cancel"""
    with cpu_emulation_stream_rows():
        m = _model()
        check_cancel(*cancel_scenario(m, inputs, gold))


def test_finish_wins_over_cancel(gold, inputs):
    """a request cancelled after the first hand-out but finished at the very next poll is delivered, not cancelled:
    requests 0 and 1 (the fixture's rows 11 and 10, set A) stop at steps 1 and 2, poll 1"""
    from easevoice_trainer_amd.auto_reg.t2s_infer import StreamControl

    d, rows = inputs, [11, 10, 0]
    a = dict(gold["sets"][0]["args"], early_stop_num=gold["early_stop_num"], slots=3, poll=1)
    reqs = [(d["x"][r], d["bert"][r], d["prompts"][r]) for r in rows]
    ctl, got = StreamControl(), []
    with cpu_emulation_stream_rows():
        m = _model()
        for item in m.decode_stream(reqs, noise=d["q"][:, rows].contiguous(), control=ctl, **a):
            got.append(item)
            if len(got) == 1:
                assert item[0] == 0
                ctl.cancel(1)
                ctl.cancel(2)
        ev = m._infer().stream_stats["events"]
    assert [r for r, _y, _i in got] == [0, 1, 2]
    y1, i1 = gold["sets"][0]["y"][10].long(), gold["sets"][0]["idx"][10]
    assert got[1][2] == i1 and torch.equal(got[1][1].long(), y1)
    assert got[2][1] is None
    assert [(k, r) for k, _s, r, _slot in ev if k != "admit"] == [("finish", 0), ("finish", 1), ("cancel", 2)]
    assert ev[-1][1] == ev[-2][1]               # same poll: one finished, the other was cancelled

"""CPU: the host side of continuous batching (auto_reg/t2s_infer.py StreamSession / decode_stream) with the launches
emulated on the session's buffers and per-row counters (tests/cpu_emu_stream.py): the reference's token lists for 20 and
36 texts (tests/golden/s1_batch_infer_rows.pt) through 5, 8 and 32 refilled slots, the admission protocol, the order of
hand-out and the capacity checks."""
import os
import sys

import pytest
import torch
import yaml

from cpu_emu_stream import cpu_emulation_stream
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


def _gold():
    return {c["args"]["R"]: c for c in torch.load(os.path.join(HERE, "golden", "s1_batch_infer_rows.pt"),
                                                  weights_only=False)["cases"]}


def _check_events(events, R, slots):
    """replays the admission log: a request only ever enters a slot that is free, every request enters and leaves once"""
    busy, admitted, finished = {}, [], []
    for kind, _step, r, slot in events:
        if kind == "admit":
            assert slot not in busy and 0 <= slot < slots, (r, slot, busy)
            busy[slot] = r
            admitted.append(r)
        else:
            assert busy.pop(slot) == r
            finished.append(r)
        assert len(busy) <= slots
    assert admitted == list(range(R)) and sorted(finished) == list(range(R)) and not busy


@pytest.mark.parametrize("R,slots", [(36, 8), (36, 32), (20, 5)])
def test_refill_matches_reference_tokens(R, slots):
    """every text comes out token for token as the reference's infer_panel_batch_infer decodes it, although its row was
    admitted at some later step into whichever slot was free (rows stop at steps 1..13, two at the early stop).  With 5
    or 8 slots the queue drains over at least three admission rounds; 36 texts in 32 slots need exactly two (the four
    waiting texts fit the slots the first poll frees)"""
    from make_golden_s1_rows import rows_inputs

    gold = _gold()[R]
    d = rows_inputs(R)
    a = {k: v for k, v in gold["args"].items() if k != "R"}
    with cpu_emulation_stream():
        m = _model()
        ys, idxs = m.infer_panel_batch_infer_refill(d["x"], d["x_lens"], d["prompts"], d["bert"], slots=slots,
                                                    noise=d["q"], **a)
        st = m._infer().stream_stats
    assert idxs == gold["idx"], (idxs, gold["idx"])
    assert len(ys) == R
    for r, (y, g) in enumerate(zip(ys, gold["y"])):
        assert torch.equal(y.long(), g.long()), r
    assert st["admissions"] >= (3 if slots < 32 else 2) and sum(st["admitted"]) == R and st["admitted"][0] == slots
    _check_events(st["events"], R, slots)


def test_stream_yields_in_completion_order():
    """decode_stream hands a row out at the poll after it stops: a row stopping at step 1 leaves before a row of the
    first admission that runs to the early stop; every request comes out exactly once.  The fixture's rows are sorted
    by length of life, so the requests are queued in an order that puts its last row (one step) between its first."""
    from make_golden_s1_rows import rows_inputs

    gold = _gold()[36]
    d = rows_inputs(36)
    a = {k: v for k, v in gold["args"].items() if k != "R"}
    assert gold["idx"][0] == a["early_stop_num"] and gold["idx"][35] == 0, gold["idx"]
    perm = [0, 35] + list(range(1, 35))               # request i is the fixture's row perm[i], and reads its noise column
    with cpu_emulation_stream():
        m = _model()
        reqs = [(d["x"][r], d["bert"][r], d["prompts"][r]) for r in perm]
        out = list(m.decode_stream(reqs, slots=8, noise=d["q"][:, perm], poll=1, **a))
    order = [i for i, _y, _idx in out]
    assert sorted(order) == list(range(36))
    for i, y, idx in out:
        assert idx == gold["idx"][perm[i]] and torch.equal(y.long(), gold["y"][perm[i]].long()), i
    assert order.index(1) < order.index(0)            # both admitted in the first round into slots 1 and 0
    assert order[0] == 1


def test_stream_per_request_limits_and_generator_input():
    """a lazy iterable with explicit capacity and per-request early stops: each request ends at its own limit"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(20)
    lims = [2 + r % 4 for r in range(10)]
    gen = ((d["x"][r], d["bert"][r], d["prompts"][r], lims[r]) for r in range(10))
    with cpu_emulation_stream():
        m = _model()
        out = {r: (y, i) for r, y, i in m.decode_stream(gen, slots=3, noise=d["q"], top_k=1100, top_p=1, early_stop_num=8,
                                                        max_text_len=max(int(x.numel()) for x in d["x"]),
                                                        max_prompt_len=d["prompts"].size(1))}
    assert sorted(out) == list(range(10))
    P = d["prompts"].size(1)
    for r, (y, i) in out.items():
        assert i <= lims[r] and y.numel() <= P + lims[r]
        assert torch.equal(y[:P].long(), d["prompts"][r].long())


def test_stream_capacity_errors():
    from make_golden_s1_rows import rows_inputs
    from easevoice_trainer_amd.auto_reg import t2s_infer as TI
    from easevoice_trainer_amd.hip.lib import EvtError

    d = rows_inputs(20)
    reqs = [(d["x"][r], d["bert"][r], d["prompts"][r]) for r in range(6)]
    longest = max(int(q[0].numel()) for q in reqs)
    launched = []
    with cpu_emulation_stream():
        m = _model()
        orig = TI.StreamSession.__init__

        def counted(self, *a, **k):
            launched.append(1)
            orig(self, *a, **k)

        TI.StreamSession.__init__ = counted
        try:
            with pytest.raises(EvtError, match="does not fit"):      # a list: checked as a whole before anything is launched
                m.decode_stream(reqs, slots=4, noise=d["q"], early_stop_num=3, max_text_len=longest - 1)
            with pytest.raises(EvtError, match="max_text_len"):
                m.decode_stream(iter(reqs), slots=4, noise=d["q"], early_stop_num=3)
            with pytest.raises(EvtError, match="slots"):
                m.decode_stream(reqs, slots=33, noise=d["q"], early_stop_num=3)
            assert not launched
            # a lazy iterable: the request that does not fit raises when it is pulled, before its admission
            short = [q for q in reqs if int(q[0].numel()) < longest]
            lazy = iter(short[:1] + [q for q in reqs if int(q[0].numel()) == longest][:1])
            g = m.decode_stream(lazy, slots=1, noise=d["q"], early_stop_num=3, max_text_len=longest - 1,
                                max_prompt_len=d["prompts"].size(1))
            assert next(g)[0] == 0
            with pytest.raises(EvtError, match="request 1 .*does not fit"):
                next(g)
            assert m._infer().stream_stats["admissions"] == 1
        finally:
            TI.StreamSession.__init__ = orig

"""CPU: stream sessions of more than 32 slots (decode_stream(..., wide=True), auto_reg/t2s_infer.py) with the launches
emulated on the session's buffers (tests/cpu_emu_stream.py).  The host loop is sized by the slot count alone: the
reference's token lists (tests/golden/s1_batch_infer_rows.pt) through 64 slots, 100 texts through 128, 48 and 32 slots
with identical tokens, candidates up to the slot count, the bounds, the memory check and the pipeline's keyword."""
import os
import sys
from types import SimpleNamespace

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


def _stream(m, d, slots, **kw):
    """all texts of d through decode_stream itself (infer_panel_batch_infer_refill clamps the slots to the number of
    texts), in input order; the session made for the stream has exactly `slots` rows"""
    R = len(d["x"])
    ys, idxs = [None] * R, [None] * R
    for r, y, i in m.decode_stream([(d["x"][r], d["bert"][r], d["prompts"][r]) for r in range(R)], slots=slots,
                                   wide=slots > 32, **kw):
        ys[r], idxs[r] = y, i
    inf = m._infer()
    assert inf._sessions[inf._wide[-1]].B == slots
    return ys, idxs


def test_reference_tokens_through_64_slots():
    """the 36 texts of the reference fixture in ONE admission of a 64-slot session: the reference's tokens and indices"""
    from make_golden_s1_rows import rows_inputs

    gold = {c["args"]["R"]: c for c in torch.load(os.path.join(HERE, "golden", "s1_batch_infer_rows.pt"),
                                                  weights_only=False)["cases"]}[36]
    d = rows_inputs(36)
    a = {k: v for k, v in gold["args"].items() if k != "R"}
    with cpu_emulation_stream():
        m = _model()
        # the list form clamps the slots to the number of texts; the stream itself keeps all 64
        reqs = [(d["x"][r], d["bert"][r], d["prompts"][r]) for r in range(36)]
        out = {r: (y, i) for r, y, i in m.decode_stream(reqs, slots=64, wide=True, noise=d["q"], **a)}
        st = m._infer().stream_stats
        assert m._infer()._sessions[m._infer()._wide[-1]].B == 64
    assert [out[r][1] for r in range(36)] == gold["idx"]
    for r, g in enumerate(gold["y"]):
        assert torch.equal(out[r][0].long(), g.long()), r
    assert st["admissions"] == 1 and st["admitted"] == [36]
    _check_events(st["events"], 36, 64)


@pytest.fixture(scope="module")
def hundred():
    """100 texts with their noise table through 32 slots: the run the wider sessions are compared with"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(100)
    kw = dict(noise=d["q"], top_k=1100, top_p=1, early_stop_num=3)
    with cpu_emulation_stream():
        m = _model()
        ys, idxs = _stream(m, d, 32, **kw)
        adm = list(m._infer().stream_stats["admitted"])
    assert adm[0] == 32 and sum(adm) == 100 and len(ys) == 100 and len(set(idxs)) > 2
    return d, kw, ys, idxs


@pytest.mark.parametrize("slots", [128, 48])
def test_100_texts_same_tokens_as_through_32_slots(hundred, slots):
    """a row's tokens do not depend on the number of slots: a session of 128 slots takes the 100 texts in one admission
    and keeps 28 rows idle, 48 slots take 48 first, and both give the tokens and indices of the 32-slot session"""
    d, kw, ys, idxs = hundred
    with cpu_emulation_stream():
        m = _model()
        y2, i2 = _stream(m, d, slots, **kw)
        st = m._infer().stream_stats
    assert st["admitted"] == [100] if slots == 128 else (st["admitted"][0] == 48 and sum(st["admitted"]) == 100)
    assert i2 == idxs
    for r in range(100):
        assert torch.equal(ys[r], y2[r]), r
    _check_events(st["events"], 100, slots)


def test_lazy_iterable_wide():
    """a lazy iterable with explicit capacity in a 40-slot session: every request at its own limit"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(50)
    lims = [2 + r % 3 for r in range(50)]
    gen = ((d["x"][r], d["bert"][r], d["prompts"][r], lims[r]) for r in range(50))
    with cpu_emulation_stream():
        m = _model()
        out = {r: (y, i) for r, y, i in m.decode_stream(gen, slots=40, wide=True, noise=d["q"], top_k=1100, top_p=1,
                                                        early_stop_num=5,
                                                        max_text_len=max(int(x.numel()) for x in d["x"]),
                                                        max_prompt_len=d["prompts"].size(1))}
        st = m._infer().stream_stats
    assert sorted(out) == list(range(50)) and st["admitted"][0] == 40 and sum(st["admitted"]) == 50
    P = d["prompts"].size(1)
    for r, (y, i) in out.items():
        assert i <= lims[r] and y.numel() <= P + lims[r] and torch.equal(y[:P].long(), d["prompts"][r].long())
    _check_events(st["events"], 50, 40)


def test_slot_bounds():
    """129 slots with wide, 33 without, 0 either way: EvtError before any session is made"""
    from make_golden_s1_rows import rows_inputs
    from easevoice_trainer_amd.auto_reg import t2s_infer as TI
    from easevoice_trainer_amd.hip.lib import EvtError

    assert TI.T2SInfer.STREAM_ROWS == 128 and TI.T2SInfer.WIDE_ROWS == 32
    d = rows_inputs(20)
    reqs = [(d["x"][r], d["bert"][r], d["prompts"][r]) for r in range(6)]
    made = []
    with cpu_emulation_stream():
        m = _model()
        orig = TI.StreamSession.__init__

        def counted(self, *a, **k):
            made.append(1)
            orig(self, *a, **k)

        TI.StreamSession.__init__ = counted
        try:
            kw = dict(noise=d["q"], early_stop_num=3)
            with pytest.raises(EvtError, match=r"slots must be 1\.\.128, got 129"):
                m.decode_stream(reqs, slots=129, wide=True, **kw)
            with pytest.raises(EvtError, match=r"slots must be 1\.\.128, got 0"):
                m.decode_stream(reqs, slots=0, wide=True, **kw)
            with pytest.raises(EvtError, match=r"slots must be 1\.\.32, got 0"):
                m.decode_stream(reqs, slots=0, **kw)
            with pytest.raises(EvtError, match=r"slots must be 1\.\.32, got 33"):
                m.decode_stream(reqs, slots=33, wide=False, **kw)
            with pytest.raises(EvtError, match=r"slots must be 1\.\.128, got 129"):
                list(m.score_stream(reqs, [[1, 2]] * 6, slots=129, wide=True))
            assert not made
        finally:
            TI.StreamSession.__init__ = orig


def test_wide_session_memory_check(monkeypatch):
    """a session of more than 32 slots on a GPU device is refused, with the bytes named and before anything is
    allocated, when its cache needs more than half of the free memory -- the device's plus what torch's allocator holds
    unused, counted after the least recently used session has made room; 32 slots are not asked"""
    from easevoice_trainer_amd.auto_reg import t2s_infer as TI
    from easevoice_trainer_amd.hip.lib import EvtError

    m = _model()
    inf = m._infer()
    need = 2 * m.num_layers * 64 * 512 * m.model_dim * 2            # bf16, Lmax rounded up to 512
    made, asked, held = [], [], []
    monkeypatch.setattr(TI, "StreamSession", lambda *a, **k: made.append(a) or SimpleNamespace())
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda dev=None: 5000)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda dev=None: 4000)       # 1000 bytes cached and unused
    for free, ok in ((2 * need - 1001, False), (2 * need - 1000, True)):
        def info(dev, free=free):
            asked.append(dev)
            held.append(len(inf._sessions))
            return free, 10 * free

        monkeypatch.setattr(torch.cuda, "mem_get_info", info)
        if ok:
            inf.stream_session(64, 24, 100, 50, torch.bfloat16, "cuda:0")
            assert len(made) == 1
        else:
            with pytest.raises(EvtError, match=f"64 slots.*{need} bytes.*{free + 1000} bytes free"):
                inf.stream_session(64, 24, 100, 50, torch.bfloat16, "cuda:0")
            assert not made and not inf._sessions and not inf._wide
    n = len(asked)
    inf.stream_session(32, 24, 100, 50, torch.bfloat16, "cuda:0")
    inf.stream_session(64, 24, 100, 50, torch.bfloat16, "cpu")
    assert len(asked) == n and len(made) == 3 and len(inf._sessions) == 2      # WIDE_SESSIONS: one was dropped
    # a third wide session: the oldest is dropped BEFORE free memory is read
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev: (asked.append(dev), held.append(len(inf._sessions)),
                                                                 (4 * need, 40 * need))[2])
    inf.stream_session(96, 24, 100, 50, torch.bfloat16, "cuda:0")
    assert len(asked) == n + 1 and held[-1] == 1 and len(inf._sessions) == 2


def test_refill_passes_wide_and_clamps_slots(monkeypatch):
    """infer_panel_batch_infer_refill hands `wide` to decode_stream with the slots clamped to the number of texts"""
    from make_golden_s1_rows import rows_inputs
    from easevoice_trainer_amd.auto_reg import t2s_infer as TI

    d = rows_inputs(40)
    seen = []
    monkeypatch.setattr(TI.T2SInfer, "decode_stream",
                        lambda self, reqs, **kw: seen.append((len(reqs), kw["slots"], kw["wide"])) or iter(()))
    m = _model()
    args = (d["x"], d["x_lens"], d["prompts"], d["bert"])
    m.infer_panel_batch_infer_refill(*args, slots=128, wide=True)
    m.infer_panel_batch_infer_refill(*args, slots=36, wide=True)
    m.infer_panel_batch_infer_refill(*args)
    assert seen == [(40, 40, True), (40, 36, True), (40, 32, False)]


def test_candidates_up_to_the_slot_count():
    """2 requests with n = 40 in 64 slots ([steps][R][C][V] table): 40 outputs per request, candidate 0 is the request's
    n = 1 run; n = 65 is refused"""
    from make_golden_s1_rows import rows_inputs
    from easevoice_trainer_amd.hip.lib import EvtError

    d = rows_inputs(20)
    q4 = torch.empty(6, 2, 40, 1025).exponential_(1, generator=torch.Generator().manual_seed(5))
    reqs = [(d["x"][r], d["bert"][r], d["prompts"][r]) for r in range(2)]
    kw = dict(top_k=1100, top_p=1, early_stop_num=20)
    with cpu_emulation_stream():
        m = _model()
        outs = list(m.decode_stream(reqs, slots=64, wide=True, n=40, noise=q4, **kw))
        st = m._infer().stream_stats
        assert st["prefill_rows"] == [1, 1] and st["admitted"] == [40, 40]      # the second request waits for 40 slots
        one = list(m.decode_stream(reqs, slots=64, wide=True, noise=q4[:, :, 0].contiguous(), **kw))
        with pytest.raises(EvtError, match=r"n = 65 must be 1\.\.slots = 64"):
            m.decode_stream(reqs, slots=64, wide=True, n=65, noise=q4, **kw)
    for r in range(2):
        mine = [o for o in outs if o.request == r]
        assert sorted(o.candidate for o in mine) == list(range(40))
        assert len({tuple(o.y.tolist()) for o in mine}) > 1
    c0 = {o.request: o for o in outs if o.candidate == 0}
    assert sorted(r for r, _y, _i in one) == [0, 1]
    for r, y, idx in one:
        assert idx == c0[r].idx and torch.equal(y, c0[r].y), r


def test_synthesize_stream_passes_wide():
    """synthesize_stream(slots=64, wide=True) opens decode_stream with both values (70 fragments, stub voices)"""
    from easevoice_trainer_amd.inference.pipeline import synthesize_stream

    seen = []

    def decode_stream(reqs, **kw):
        seen.append((len(reqs), kw))
        return iter([(r, torch.arange(20), 5) for r in range(len(reqs))])

    t2s = SimpleNamespace(model=SimpleNamespace(decode_stream=decode_stream), device="cpu", early_stop_num=20)
    voice = SimpleNamespace(model=SimpleNamespace(decode=lambda sem, ph, refer, speed=1.0: sem.float()))
    n = 70
    ids, bert = [torch.zeros(3, dtype=torch.long)] * n, [torch.zeros(1024, 3)] * n
    got = list(synthesize_stream(t2s, voice, ids, ids, bert, torch.zeros(1, 4, dtype=torch.long), [], slots=64, wide=True))
    assert len(got) == n and len(seen) == 1
    assert seen[0][0] == n and seen[0][1]["slots"] == 64 and seen[0][1]["wide"] is True
    list(synthesize_stream(t2s, voice, ids, ids, bert, torch.zeros(1, 4, dtype=torch.long), [], slots=20))
    assert seen[1][1]["slots"] == 20 and seen[1][1]["wide"] is False

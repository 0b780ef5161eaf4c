"""CPU: candidates per request (n) and per-token log-probabilities in a refilled s1 decode session
(auto_reg/t2s_infer.py decode_stream / StreamOutput), launches emulated on the session's buffers
(tests/cpu_emu_stream_lp.py).  Reference: tests/golden/s1_logprobs.pt, the reference's infer_panel_batch_infer on
4 texts x 3 candidates with the model's and the sampler's log-probability of every drawn token; candidate c of request r
is the fixture's row 3r + c."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import yaml

from cpu_emu_stream_lp import cpu_emulation_stream_lp
from util_fill import fill_module

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

# max |log-probability - fixture| measured with this file on the CPU over all steps, 7 and 12 slots: 2.4e-6 (set A;
# set D 1.9e-6).  The two sides differ in the fp32 summation order of the same arithmetic; the bound is 4 x that
LP_TOL = 9.6e-6


def _model():
    from easevoice_trainer_amd.auto_reg.t2s_model import Text2SemanticDecoder

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "gpt.yaml")))
    m = Text2SemanticDecoder(cfg)
    fill_module(m, 3)
    m.eval()
    return m


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(HERE, "golden", "s1_logprobs.pt"), weights_only=False)


@pytest.fixture(scope="module")
def inputs(gold):
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(gold["texts"] * gold["candidates"])
    d["q4"] = d["q"].view(d["q"].size(0), gold["texts"], gold["candidates"], -1)      # [steps][R][C][V]
    return d


def requests(d, rows, dev="cpu"):
    return [(d["x"][r].to(dev), d["bert"][r].to(dev), d["prompts"][r].to(dev)) for r in rows]


def check_against_fixture(outs, gold, name, tol, dev_note=""):
    """outs: StreamOutputs of the four requests with n = 3.  Tokens and indices exactly; returns the largest absolute
    log-probability difference after asserting it against tol (None: measure only)"""
    T, Cn, g = gold["texts"], gold["candidates"], gold["sets"][name]
    assert sorted((o.request, o.candidate) for o in outs) == [(r, c) for r in range(T) for c in range(Cn)]
    worst = 0.0
    for o in outs:
        row = Cn * o.request + o.candidate
        assert o.idx == g["idx"][row], (name, row, o.idx, g["idx"][row])
        assert torch.equal(o.y.cpu().long(), g["y"][row].long()), (name, row)
        lp, ref = o.logprobs.cpu(), g["logprobs"][row]
        assert lp.dtype == torch.float32 and lp.shape == ref.shape, (name, row, lp.shape, ref.shape)
        # one row per step taken: the tokens kept, then the step that stopped the candidate
        assert lp.size(0) == o.y.numel() - 12 + 1
        assert torch.isfinite(lp).all() and bool((lp <= 1e-6).all())
        worst = max(worst, float((lp - ref).abs().max()))
    print(f"max |logprob - fixture| set {name}{dev_note}: {worst:.3e}")
    if tol is not None:
        assert worst <= tol, (name, worst, tol)
    return worst


@pytest.mark.parametrize("name", ["A", "D"])
@pytest.mark.parametrize("slots", [7, 12])
def test_candidates_match_reference_tokens_and_logprobs(gold, inputs, slots, name):
    """four requests with n = 3 and the 4-D table through 7 slots (two admissions at least) and through 12 (one): tokens
    and indices are the fixture's, candidate for candidate; log-probabilities within LP_TOL = 9.6e-6, four times the
    2.4e-6 measured here on the CPU against the fixture (fp32 summation order of the same arithmetic)"""
    g = gold["sets"][name]
    with cpu_emulation_stream_lp():
        m = _model()
        outs = list(m.decode_stream(requests(inputs, range(4)), slots=slots, n=3, logprobs=True, noise=inputs["q4"],
                                    early_stop_num=gold["early_stop_num"], **g["args"]))
        st = m._infer().stream_stats
    from easevoice_trainer_amd.auto_reg.t2s_infer import StreamOutput

    assert all(isinstance(o, StreamOutput) for o in outs)
    check_against_fixture(outs, gold, name, LP_TOL)
    # admission accounting: prefill_rows counts the unique requests of an admission, admitted its slots
    assert sum(st["prefill_rows"]) == 4 and sum(st["admitted"]) == 12
    assert st["admitted"] == [3 * k for k in st["prefill_rows"]] and st["admissions"] == len(st["prefill_rows"])
    assert st["prefill_rows"][0] == (4 if slots == 12 else 2)
    assert (st["admissions"] == 1) == (slots == 12)


def test_head_of_line(gold, inputs):
    """4 slots, requests with n = 3, 3, 1 (texts 3, 2, 0, so request 0's candidates stop at steps 3, 2 and 1): request 1
    is admitted only once three slots are free, all its candidates at one step, and request 2 never precedes it although
    a single slot was free all along"""
    d, a = inputs, gold["sets"]["A"]["args"]
    q4 = d["q4"][:, [3, 2, 0]].contiguous()
    reqs = [(*q, dict(n=k)) for q, k in zip(requests(d, [3, 2, 0]), (3, 3, 1))]
    with cpu_emulation_stream_lp():
        m = _model()
        outs = list(m.decode_stream(reqs, slots=4, noise=q4, poll=1, early_stop_num=gold["early_stop_num"], **a))
        st = m._infer().stream_stats
    assert sorted((o.request, o.candidate) for o in outs) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0)]
    assert all(o.logprobs is None and o.y is not None for o in outs)
    busy, order, admit_step = set(), [], {}
    for kind, step, r, slot in st["events"]:
        if kind == "admit":
            assert slot not in busy
            busy.add(slot)
            order.append(r)
            admit_step.setdefault(r, set()).add(step)
        else:
            busy.remove(slot)
    assert order == [0, 0, 0, 1, 1, 1, 2]
    assert admit_step[0] == {0} and len(admit_step[1]) == 1
    s1 = min(admit_step[1])
    finished0 = [step for kind, step, r, _slot in st["events"] if kind == "finish" and r == 0]
    assert s1 == sorted(finished0)[1] and s1 > min(finished0)     # the second finish of request 0 frees the third slot
    assert min(admit_step[2]) >= s1
    assert st["prefill_rows"][0] == 1 and st["admitted"][0] == 3
    # the fixture's rows: request 0 is text 3 with columns 9..11, request 1 text 2 with columns 6..8
    g = gold["sets"]["A"]
    for o in outs:
        row = {0: 9, 1: 6, 2: 0}[o.request] + o.candidate
        assert o.idx == g["idx"][row] and torch.equal(o.y.long(), g["y"][row].long()), row


def test_candidate_zero_is_the_single_request_and_defaults_are_tuples(gold, inputs):
    """candidate 0 of an n = 3 stream equals the n = 1 stream's tokens for every request (3-D table of the candidate-0
    columns); and a stream with n = 1, logprobs=False yields plain 3-tuples, the existing rows fixture's tokens"""
    from make_golden_s1_rows import rows_inputs
    from easevoice_trainer_amd.auto_reg.t2s_infer import StreamOutput

    d, a = inputs, gold["sets"]["A"]["args"]
    kw = dict(slots=7, early_stop_num=gold["early_stop_num"], **a)
    with cpu_emulation_stream_lp():
        m = _model()
        three = [o for o in m.decode_stream(requests(d, range(4)), n=3, noise=d["q4"], **kw)]
        one = list(m.decode_stream(requests(d, range(4)), noise=d["q4"][:, :, 0].contiguous(), **kw))
        assert m._infer().stream_stats["prefill_rows"] == m._infer().stream_stats["admitted"]
        rows = torch.load(os.path.join(HERE, "golden", "s1_batch_infer_rows.pt"), weights_only=False)["cases"][0]
        ra = dict(rows["args"])
        R = ra.pop("R")
        dr = rows_inputs(R)
        plain = list(m.decode_stream(requests(dr, range(R)), slots=5, noise=dr["q"], **ra))
        ys, idxs = m.infer_panel_batch_infer_refill(dr["x"], dr["x_lens"], dr["prompts"], dr["bert"], slots=5,
                                                    noise=dr["q"], **ra)
    assert all(type(t) is tuple and len(t) == 3 for t in one + plain)
    assert all(isinstance(o, StreamOutput) and o.logprobs is None for o in three)
    c0 = {o.request: o for o in three if o.candidate == 0}
    assert sorted(r for r, _y, _i in one) == sorted(c0) == list(range(4))
    for r, y, idx in one:
        assert idx == c0[r].idx and torch.equal(y, c0[r].y), r
    assert any(not torch.equal(o.y, c0[o.request].y) for o in three if o.candidate)
    assert sorted(r for r, _y, _i in plain) == list(range(R))
    for r, y, idx in plain:
        assert idx == rows["idx"][r] == idxs[r] and torch.equal(y.long(), rows["y"][r].long()) and torch.equal(y, ys[r]), r


def test_list_form_returns_logprobs(gold, inputs):
    """infer_panel_batch_infer_refill(logprobs=True) returns (ys, idxs, lps): text r with the 3-D table of the
    candidate-0 columns is the fixture's row 3r"""
    d, g = inputs, gold["sets"]["D"]
    with cpu_emulation_stream_lp():
        m = _model()
        ys, idxs, lps = m.infer_panel_batch_infer_refill(d["x"][:4], d["x_lens"][:4], d["prompts"][:4], d["bert"][:4],
                                                         slots=3, noise=d["q4"][:, :, 0].contiguous(), logprobs=True,
                                                         early_stop_num=gold["early_stop_num"], **g["args"])
    for r in range(4):
        assert idxs[r] == g["idx"][3 * r] and torch.equal(ys[r].long(), g["y"][3 * r].long())
        assert float((lps[r] - g["logprobs"][3 * r]).abs().max()) <= LP_TOL


@pytest.mark.parametrize("case", ["zero", "over_slots", "fraction", "request_over_slots", "no_candidate_dim",
                                  "over_table", "own_n_in_plain_stream"])
@pytest.mark.parametrize("lazy", [False, True], ids=["list", "generator"])
def test_bad_n_is_refused(gold, inputs, case, lazy):
    """n = 0, n > slots, a non-integer n, a request's own n > slots, n = 2 with a 3-D table and n above the table's
    candidate dimension raise EvtError: for a list before any StreamSession is made, for a lazy iterable when the
    request is drawn (session-wide values at the call; requests 0 and 1 with two candidates each are running by the
    time request 2 is drawn).  own_n_in_plain_stream: n = 1 session-wide without logprobs, request 2 asks for n = 2 in
    its dict.  A list sees that before it opens and yields StreamOutputs throughout; a lazy iterable has fixed the
    3-tuple form by then and refuses the request when it is drawn (requests 0 and 1 are running)"""
    from easevoice_trainer_amd.auto_reg import t2s_infer as TI
    from easevoice_trainer_amd.hip.lib import EvtError

    d = inputs
    kw = dict(slots=4, n=2, noise=d["q4"], top_k=1100, top_p=1, early_stop_num=3, poll=1)
    reqs, per_request, match = requests(d, range(4)), False, "n = "
    if case == "zero":
        kw["n"] = 0
    elif case == "over_slots":
        kw["n"] = 5
    elif case == "fraction":
        kw["n"] = 1.5
    elif case == "request_over_slots":
        reqs[2] = (*reqs[2], dict(n=5))
        per_request, match = True, "request 2: n = 5"
    elif case == "no_candidate_dim":
        kw.update(noise=d["q"][:, :4].contiguous())
        per_request, match = True, "request 0: .*the noise table has no candidate dimension"
    elif case == "own_n_in_plain_stream":
        kw.update(n=1, slots=2)        # two slots: requests 0 and 1 fill them before request 2 is drawn
        reqs[2] = (*reqs[2], dict(n=2))
        per_request, match = True, "request 2: n = 2 in a lazy stream"
    else:
        reqs[2] = (*reqs[2], dict(n=4))
        per_request, match = True, "request 2: .*3 candidates"
    made = []
    with cpu_emulation_stream_lp():
        m = _model()
        orig = TI.StreamSession.__init__

        def counted(self, *a, **k):
            made.append(1)
            orig(self, *a, **k)

        TI.StreamSession.__init__ = counted
        try:
            if not lazy and case == "own_n_in_plain_stream":
                outs = list(m.decode_stream(reqs, **kw))
                assert all(isinstance(o, TI.StreamOutput) and o.logprobs is None for o in outs)
                assert sorted((o.request, o.candidate) for o in outs) == [(0, 0), (1, 0), (2, 0), (2, 1), (3, 0)]
            elif not lazy:
                with pytest.raises(EvtError, match=match):
                    m.decode_stream(reqs, **kw)
                assert not made
            elif not per_request:
                with pytest.raises(EvtError, match=match):
                    m.decode_stream(iter(reqs), max_text_len=24, max_prompt_len=12, **kw)
                assert not made
            else:
                g = m.decode_stream(iter(reqs), max_text_len=24, max_prompt_len=12, **kw)
                with pytest.raises(EvtError, match=match):
                    list(g)
                admits = [r for kind, _s, r, _slot in m._infer().stream_stats["events"] if kind == "admit"]
                assert admits == {"no_candidate_dim": [], "own_n_in_plain_stream": [0, 1]}.get(case, [0, 0, 1, 1])
        finally:
            TI.StreamSession.__init__ = orig


def test_cancel_with_candidates(gold, inputs):
    """4 slots, poll 1, set A.  Request 0 (n = 1) stops at step 1; request 1 has three candidates of which candidate 1
    stops at step 2; requests 2 and 3 (n = 3) wait.  After the first hand-out requests 1 and 3 are cancelled: at the
    next poll candidate 1 of request 1 is delivered (finish wins), candidates 0 and 2 come as None, all three slots are
    free for request 2 in that poll's admission, and request 3 gives three None outputs without a prompt pass"""
    from easevoice_trainer_amd.auto_reg.t2s_infer import StreamControl

    d, a = inputs, gold["sets"]["A"]["args"]
    q = d["q"]
    cols = [[11, 11, 11], [3, 10, 0], [4, 5, 6], [7, 8, 9]]          # columns stop at step: 11 -> 1, 10 -> 2, others later
    q4 = torch.stack([q[:, c] for c in cols], dim=1).contiguous()
    reqs = requests(d, [3, 1, 2, 0])
    reqs[0] = (*reqs[0], dict(n=1))
    kw = dict(slots=4, n=3, noise=q4, poll=1, early_stop_num=gold["early_stop_num"], **a)
    with cpu_emulation_stream_lp():
        m = _model()
        plain = {(o.request, o.candidate): o for o in m.decode_stream(reqs, **kw)}
        ctl, got = StreamControl(), []
        for o in m.decode_stream(reqs, control=ctl, logprobs=True, **kw):
            got.append(o)
            if len(got) == 1:
                assert (o.request, o.candidate) == (0, 0) and o.y is not None
                ctl.cancel(1)
                ctl.cancel(3)
        st = m._infer().stream_stats
    by = {(o.request, o.candidate): o for o in got}
    assert sorted(by) == [(0, 0)] + [(r, c) for r in (1, 2, 3) for c in range(3)] and len(got) == 10
    assert by[1, 1].y is not None and torch.equal(by[1, 1].y, plain[1, 1].y) and by[1, 1].idx == plain[1, 1].idx == 1
    assert by[1, 1].logprobs.shape == (3, 2)
    for key in [(1, 0), (1, 2), (3, 0), (3, 1), (3, 2)]:
        assert by[key].y is None and by[key].idx is None and by[key].logprobs is None, key
    for c in range(3):
        assert torch.equal(by[2, c].y, plain[2, c].y) and by[2, c].idx == plain[2, c].idx
        assert by[2, c].logprobs.size(0) == by[2, c].y.numel() - 12 + 1
    ev = st["events"]
    assert not any(kind == "admit" and r == 3 for kind, _s, r, _slot in ev)
    assert [(k, r, slot) for k, _s, r, slot in ev if k == "cancel" and r == 3] == [("cancel", 3, None)]
    poll2 = [(k, r, slot) for k, s, r, slot in ev if s == 2 and r != 3]
    assert sorted(e for e in poll2 if e[0] != "admit") == [("cancel", 1, 1), ("cancel", 1, 3), ("finish", 1, 2)]
    assert [e for e in poll2 if e[0] == "admit"] == [("admit", 2, 0), ("admit", 2, 1), ("admit", 2, 2)]
    assert st["prefill_rows"] == [2, 1] and st["admitted"] == [4, 3]


def test_pipeline_candidates(gold):
    """synthesize_stream(candidates=2): choose is called once per fragment with that fragment's two StreamOutputs in
    candidate order, log-probabilities on; only the chosen take reaches the s2 decoder (its calls are counted); a
    missing choose raises"""
    from make_golden_s1_inputs import pipeline_inputs
    from easevoice_trainer_amd.inference.pipeline import synthesize_stream

    d = pipeline_inputs()
    q2 = torch.empty(32, 2, 1025).exponential_(1, generator=torch.Generator().manual_seed(9))
    q2[5, 0, 1024] = 1e-30
    q2[11, 1, 1024] = 1e-30
    q4 = torch.stack([d["q"], q2], dim=2).contiguous()
    calls, asked = [], []

    def decode(sem, phones, refer, speed=1.0):
        calls.append(sem[0, 0].clone())
        return sem.float()

    def choose(i, outs):
        asked.append((i, outs))
        return 1 - i

    voice = SimpleNamespace(model=SimpleNamespace(decode=decode))
    with cpu_emulation_stream_lp():
        m = _model()
        t2s = SimpleNamespace(model=m, device="cpu", early_stop_num=20)
        args = (t2s, voice, d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], [])
        kw = dict(top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35, sample_kwargs=dict(noise=q4, poll=2))
        with pytest.raises(ValueError, match="choose"):
            list(synthesize_stream(*args, candidates=2, **kw))
        with pytest.raises(ValueError, match="slots = 1 cannot hold the 2 candidates"):
            list(synthesize_stream(*args, candidates=2, choose=choose, slots=1, **kw))
        assert not calls and not asked
        got = list(synthesize_stream(*args, candidates=2, choose=choose, **kw))
    assert sorted(i for i, _w in got) == [0, 1] and sorted(i for i, _o in asked) == [0, 1] and len(calls) == 2
    stops = {(0, 0): 14, (0, 1): 5, (1, 0): 9, (1, 1): 11}
    for i, outs in asked:
        assert [o.candidate for o in outs] == [0, 1] and all(o.request == i for o in outs)
        for o in outs:
            assert o.idx == stops[i, o.candidate] - 1 and o.logprobs.shape == (stops[i, o.candidate] + 1, 2)
    for i, w in got:
        t = dict(asked)[i][1 - i]
        assert torch.equal(w, t.y[-t.idx:].float())
    assert [i for i, _w in got] == [i for i, _o in asked]

"""CPU: forced tokens ("force"), per-request seeds ("seed"), StreamControl.preempt and score_stream of a refilled s1
decode session (auto_reg/t2s_infer.py), launches emulated on the session's buffers (tests/cpu_emu_stream_force.py).
Reference: tests/golden/s1_logprobs.pt, sets A and D -- the reference's own tokens and its two log-probabilities per step
for 12 rows.  Here the 12 rows are 12 requests with n = 1: request i is text i // 3 and reads noise column i."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import yaml

from cpu_emu_stream_force import cpu_emulation_stream_force
from test_s1_stream_candidates_cpu import LP_TOL
from util_fill import fill_module

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

P = 12          # the fixture's prompt length
EOS = 1024
SLOTS = 5       # fewer slots than requests: the refills are staggered


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

    return rows_inputs(gold["texts"] * gold["candidates"])


def row_requests(d, rows, dev="cpu", opts=None):
    """one request per fixture row j in `rows`: text j // 3 and its prompt; opts: {position in rows: dict}"""
    out = []
    for k, j in enumerate(rows):
        t = j // 3
        q = (d["x"][t].to(dev), d["bert"][t].to(dev), d["prompts"][t].to(dev))
        out.append((*q, dict(opts[k])) if opts and k in opts else q)
    return out


def generated(g, j):
    """the fixture's kept tokens of row j behind the prompt"""
    return g["y"][j][P:].long()


def stopped_by_planned_eos(g, j, R=12):
    """row j drew the EOS its noise column plants: one log-probability row per step 0..stop, idx = stop - 1"""
    from make_golden_s1_rows import stop_step

    s = stop_step(j, R)
    return s is not None and g["logprobs"][j].size(0) == s + 1 and g["idx"][j] == s - 1 and generated(g, j).numel() == s


def resume_plan(g, name):
    """k_j forced tokens per row, as a token vector or None: 0, 1, half, all kept tokens (the stopping step is then
    sampled), and -- set A, rows that stop at their planned step -- all kept tokens plus the EOS (nothing is sampled)"""
    plan, kinds = {}, set()
    for j in range(12):
        gen = generated(g, j)
        G = gen.numel()
        kind = ("none", "one", "middle", "all", "all+eos")[j % 5]
        if kind == "all+eos" and not (name == "A" and stopped_by_planned_eos(g, j)):
            kind = "all"
        k = dict(none=0, one=1, middle=G // 2, all=G)[kind] if kind != "all+eos" else G
        tok = gen[:k]
        if kind == "all+eos":
            tok = torch.cat([tok, torch.tensor([EOS])])
        if kind == "middle":
            assert 1 < k < G
        kinds.add(kind)
        plan[j] = tok if tok.numel() else None
    assert kinds >= ({"none", "one", "middle", "all", "all+eos"} if name == "A" else {"none", "one", "middle", "all"})
    return plan


def check_rows(outs, g, tol, note="", rows=None):
    """outs: 3-tuples or StreamOutputs, request k <-> fixture row rows[k]; tokens and indices exactly, log-probabilities
    (when there) within tol of the fixture's; the largest difference is printed before it is asserted"""
    rows = list(range(12)) if rows is None else rows
    assert sorted(o[0] for o in outs) == list(range(len(rows)))
    worst = 0.0
    for o in outs:
        j = rows[o[0]]
        assert o[2] == g["idx"][j], (j, o[2], g["idx"][j])
        assert torch.equal(o[1].cpu().long(), g["y"][j].long()), j
        lp = getattr(o, "logprobs", None)
        if lp is not None:
            ref = g["logprobs"][j]
            assert lp.dtype == torch.float32 and lp.shape == ref.shape, (j, lp.shape, ref.shape)
            assert torch.isfinite(lp).all()
            worst = max(worst, float((lp.cpu() - ref).abs().max()))
    print(f"max |logprob - fixture|{note}: {worst:.3e}")
    assert worst <= tol, (worst, tol)
    return worst


def resume_case(m, d, gold, name, dev="cpu"):
    g = gold["sets"][name]
    plan = resume_plan(g, name)
    opts = {j: dict(force=tok) for j, tok in plan.items() if tok is not None}
    reqs = row_requests(d, range(12), dev, opts)
    return list(m.decode_stream(reqs, slots=SLOTS, logprobs=True, noise=d["q"], early_stop_num=gold["early_stop_num"],
                                **g["args"]))


@pytest.mark.parametrize("name", ["A", "D"])
def test_resume_from_forced_prefix(gold, inputs, name):
    """every request is forced over the first k of its golden tokens (k = 0, 1, half, all, all + EOS) and samples the
    rest from the fixture's noise table: y and idx are the fixture's exactly, every log-probability -- forced step or
    sampled -- within LP_TOL of test_s1_stream_candidates_cpu.py (9.6e-6: a forced step runs the arithmetic of a
    sampled one on the same tokens)"""
    with cpu_emulation_stream_force():
        m = _model()
        outs = resume_case(m, inputs, gold, name)
        st = m._infer().stream_stats
        S = m._infer()._sessions[m._infer()._wide[-1]]
        assert S.force_on and S.lp_on
    assert st["admissions"] > 1 and st["admitted"][0] == SLOTS
    check_rows(outs, gold["sets"][name], LP_TOL, note=f" resume set {name} cpu")


def score_case(m, d, gold, dev="cpu"):
    """score_stream over set A's golden tokens (plus the EOS of the rows that drew their planned one) under a noise
    table that has nothing to do with the fixture's; returns {row: (logprobs, fixture rows)}"""
    g = gold["sets"]["A"]
    toks = []
    for j in range(12):
        t = generated(g, j)
        toks.append(torch.cat([t, torch.tensor([EOS])]) if stopped_by_planned_eos(g, j) else t)
    junk = torch.empty(gold["early_stop_num"] + 2, 12, 1025).exponential_(1, generator=torch.Generator().manual_seed(77))
    got = dict(m.score_stream(row_requests(d, range(12), dev), toks, slots=SLOTS, noise=junk, **g["args"]))
    return {j: (got[j], g["logprobs"][j][:toks[j].numel()]) for j in range(12)}


def check_scores(res, tol, note=""):
    worst = 0.0
    for j, (lp, ref) in res.items():
        assert lp.dtype == torch.float32 and lp.shape == ref.shape, (j, lp.shape, ref.shape)
        worst = max(worst, float((lp.cpu() - ref).abs().max()))
    print(f"max |score - fixture|{note}: {worst:.3e}")
    assert worst <= tol, (worst, tol)


def test_score_stream_under_junk_noise(gold, inputs):
    """no noise value can change a forced row: the fixture's log-probabilities come back within LP_TOL whatever the
    table; append_eos=True scores the EOS behind the given tokens (rows 9..11 stop by their planned EOS at steps 3..1)"""
    g = gold["sets"]["A"]
    with cpu_emulation_stream_force():
        m = _model()
        res = score_case(m, inputs, gold)
        short = [j for j in (9, 10, 11) if stopped_by_planned_eos(g, j)]
        tail = dict(m.score_stream(iter(row_requests(inputs, short)), (generated(g, j) for j in short), slots=2,
                                   append_eos=True, max_text_len=24, max_prompt_len=P, **g["args"]))
    check_scores(res, LP_TOL, " set A cpu")
    assert short
    for k, j in enumerate(short):
        assert tail[k].shape == g["logprobs"][j].shape and float((tail[k] - g["logprobs"][j]).abs().max()) <= LP_TOL


def preempt_case(m, d, gold, dev="cpu", r=1):
    """set A, poll = 2, preempt(r) before the first next(); then a second stream in which r carries what it had.
    Returns (outputs of the first stream, its stats, outputs of the second)"""
    from easevoice_trainer_amd.auto_reg.t2s_infer import StreamControl

    g = gold["sets"]["A"]
    assert g["logprobs"][r].size(0) >= 5
    kw = dict(slots=SLOTS, logprobs=True, noise=d["q"], poll=2, early_stop_num=gold["early_stop_num"], **g["args"])
    ctl = StreamControl()
    ctl.preempt(r)
    first = list(m.decode_stream(row_requests(d, range(12), dev), control=ctl, **kw))
    st = m._infer().stream_stats
    part = [o for o in first if o.request == r][0]
    reqs = row_requests(d, range(12), dev, {r: dict(force=part.y[P:])})
    return first, st, list(m.decode_stream(reqs, **kw))


def check_preempt(first, st, second, g, tol, r=1, note=""):
    part = [o for o in first if o.request == r]
    assert len(part) == 1 and len(first) == 12
    part = part[0]
    # idx None with y not None marks the preempted row: step 0 plus two replays
    assert part.idx is None and part.candidate == 0
    assert torch.equal(part.y.cpu().long(), g["y"][r][:P + 3].long())
    assert part.logprobs.shape == (3, 2)
    d = float((part.logprobs.cpu() - g["logprobs"][r][:3]).abs().max())
    print(f"max |partial logprob - fixture|{note}: {d:.3e}")
    assert d <= tol
    ev = st["events"]
    pre = [e for e in ev if e[0] == "preempt"]
    assert len(pre) == 1 and pre[0][1:3] == (2, r)
    slot = pre[0][3]
    nxt = [e for e in ev if e[0] == "admit" and e[1] == 2]
    assert [e[2:] for e in nxt] == [(SLOTS, slot)]            # the freed slot goes to the next waiting request at that poll
    rest = [o for o in first if o.request != r]
    for o in rest:
        assert o.idx == g["idx"][o.request] and torch.equal(o.y.cpu().long(), g["y"][o.request].long()), o.request
    check_rows(second, g, tol, note=f" resumed{note}")


def test_preempt_hands_out_the_prefix_and_force_resumes_it(gold, inputs):
    g = gold["sets"]["A"]
    with cpu_emulation_stream_force():
        m = _model()
        first, st, second = preempt_case(m, inputs, gold)
    check_preempt(first, st, second, g, LP_TOL, note=" cpu")


def test_preempt_of_waiting_and_of_finished_requests(gold, inputs):
    """rows 11, 10 and 0 (stop at steps 1 and 2; row 0 runs to the limit) in three slots plus row 5 waiting, 3-tuple
    form, poll = 2, all four preempted before the first next(): the two that finished at that poll are delivered, row 0
    comes as (r, y, None) with P + 3 tokens, the waiting request as (r, None, None) without a prompt pass"""
    from easevoice_trainer_amd.auto_reg.t2s_infer import StreamControl

    g, rows = gold["sets"]["A"], [11, 10, 0, 5]
    q = inputs["q"][:, rows].contiguous()
    ctl = StreamControl()
    for r in range(4):
        ctl.preempt(r)
    with cpu_emulation_stream_force():
        m = _model()
        outs = list(m.decode_stream(row_requests(inputs, rows), slots=3, noise=q, poll=2, control=ctl,
                                    early_stop_num=gold["early_stop_num"], **g["args"]))
        st = m._infer().stream_stats
        S = m._infer()._sessions[m._infer()._wide[-1]]
        assert not S.force_on and not S.lp_on
    assert all(type(o) is tuple and len(o) == 3 for o in outs)
    by = {o[0]: o for o in outs}
    assert sorted(by) == [0, 1, 2, 3]
    for k in (0, 1):
        assert by[k][2] == g["idx"][rows[k]] and torch.equal(by[k][1].long(), g["y"][rows[k]].long()), k
    assert by[2][2] is None and torch.equal(by[2][1].long(), g["y"][0][:P + 3].long())
    assert by[3][1] is None and by[3][2] is None
    kinds = sorted((e[0], e[2], e[3]) for e in st["events"] if e[0] != "admit")
    assert kinds == [("cancel", 3, None), ("finish", 0, 0), ("finish", 1, 1), ("preempt", 2, 2)]
    assert st["prefill_rows"] == [3]


CASES = {
    "token_V": (dict(force=[5, 1025]), r"request 2: force\[1\] = 1025 is outside"),
    "eos_middle": (dict(force=[5, EOS, 7]), r"request 2: force\[1\] is EOS"),
    "eos_first": (dict(force=[EOS]), r"request 2: force\[0\] is EOS"),
    "over_limit": (dict(force=[1, 2, 3, 4, 5], early_stop_num=3), "request 2: 5 forced tokens, but the request's step limit is 4"),
    "over_capacity": (dict(force=[1, 2, 3, 4, 5, 6], early_stop_num=9), "request 2: 6 forced tokens, but the session's capacity"),
    "lazy_without_flag": (dict(force=[5]), "request 2: \"force\" in a lazy stream needs"),
    "bool_seed": (dict(seed=True), "request 2: seed = True"),
    "float_seed": (dict(seed=1.5), "request 2: seed = 1.5"),
    "lane_4": (dict(seed=(7, 4)), "request 2: seed lane = 4"),
    "float_force": (dict(force=[1.0, 2.0]), "request 2: force must be a 1-D integer vector"),
}


LAZY_ONLY = ("over_capacity", "lazy_without_flag")


@pytest.mark.parametrize("case,lazy", [(c, z) for c in sorted(CASES) for z in (False, True) if z or c not in LAZY_ONLY],
                         ids=lambda v: v if isinstance(v, str) else ("generator" if v else "list"))
def test_bad_force_and_seed_are_refused(inputs, case, lazy):
    """each of these raises EvtError naming request 2: for a list before any StreamSession is made, for a lazy iterable
    when the request is drawn (two slots: requests 0 and 1 are running by then).  over_capacity and lazy_without_flag
    exist for a lazy stream only: a list computes its capacity and its sampler launch from itself"""
    from easevoice_trainer_amd.auto_reg import t2s_infer as TI
    from easevoice_trainer_amd.hip.lib import EvtError

    opt, match = CASES[case]
    d = inputs
    reqs = row_requests(d, [0, 3, 6, 9], opts={2: opt})
    kw = dict(slots=2, noise=d["q"], top_k=1100, top_p=1, early_stop_num=3, poll=1)
    made = []
    with cpu_emulation_stream_force():
        m = _model()
        orig = TI.StreamSession.__init__

        def counted(self, *a, **k):
            made.append(1)
            orig(self, *a, **k)

        TI.StreamSession.__init__ = counted
        try:
            if not lazy:
                with pytest.raises(EvtError, match=match):
                    m.decode_stream(reqs, **kw)
                assert not made
            else:
                g = m.decode_stream(iter(reqs), max_text_len=24, max_prompt_len=P, forced=case != "lazy_without_flag",
                                    **kw)
                with pytest.raises(EvtError, match=match):
                    list(g)
                admits = [r for kind, _s, r, _slot in m._infer().stream_stats["events"] if kind == "admit"]
                assert admits == [0, 1]
        finally:
            TI.StreamSession.__init__ = orig


def test_pipeline_preempted_fragment_and_forced_fragment(gold):
    """synthesize_stream: a fragment preempted through the control is yielded as (index, None) and never reaches the s2
    decoder; a fragment whose fragment_sampling dict forces its first tokens decodes to the take it had without them"""
    from make_golden_s1_inputs import pipeline_inputs
    from easevoice_trainer_amd.auto_reg.t2s_infer import StreamControl
    from easevoice_trainer_amd.inference.pipeline import synthesize_stream

    d = pipeline_inputs()
    calls = []

    def decode(sem, phones, refer, speed=1.0):
        calls.append(sem[0, 0].clone())
        return sem.float()

    voice = SimpleNamespace(model=SimpleNamespace(decode=decode))
    with cpu_emulation_stream_force():
        m = _model()
        t2s = SimpleNamespace(model=m, device="cpu", early_stop_num=20)
        args = (t2s, voice, d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], [])
        kw = dict(top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35, sample_kwargs=dict(noise=d["q"], poll=2))
        reqs = [(p, b, d["prompt"].reshape(-1)) for p, b in zip(d["all_ids"], d["bert"])]
        plain = {r: (y, idx) for r, y, idx in m.decode_stream(reqs, noise=d["q"], early_stop_num=20, top_k=1100, top_p=1)}
        y1, idx1 = plain[1]
        npr = d["prompt"].numel()
        ctl = StreamControl()
        ctl.preempt(0)
        got = dict(synthesize_stream(*args, control=ctl, fragment_sampling=[None, dict(force=y1[npr:npr + 4])], **kw))
    assert got[0] is None and len(calls) == 1
    assert torch.equal(got[1], y1[-idx1:].float())

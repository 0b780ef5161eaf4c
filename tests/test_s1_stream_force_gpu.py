"""GPU: forced tokens, per-request seeds and preemption in a refilled s1 decode session.  The sampler launch with forced
steps (evt_dec_sample_embed_rows_f, csrc/s1_decode_stream.hip) against evt_dec_sample_embed_rows_lp / _p bit for bit when
nothing is forced, against a sampled step that drew the same token, and against float64 references; sessions against the
reference's tokens and log-probabilities (tests/golden/s1_logprobs.pt, fp32, graph replay and eager launches): resume from
a forced prefix, scoring under junk noise, preempt and resume; the launches of a stream without the new keys; seeds."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import yaml

from test_s1_stream_candidates_gpu import LP_TOL_GPU
from test_s1_stream_force_cpu import (P, check_preempt, check_rows, check_scores, preempt_case, resume_case, row_requests,
                                      score_case)
from util_fill import fill_module

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

IDLE, RUNNING, STOP_EOS, STOP_LIMIT = 0, 1, 2, 3
B, V, E, YMAX, NPOS, EOS = 4, 1025, 64, 24, 64, 1024
FILL = -7.0
NAMES = ("y", "rstate", "stop", "x", "probs", "logp")
SET_A = dict(top_k=1100, top_p=1.0, temperature=1.0, repetition_penalty=1.35)


def _i32(v, gpu):
    return torch.tensor(v, dtype=torch.int32, device=gpu)


def _table(rows, gpu):
    t = torch.tensor([[0.0, s["top_p"], s["temperature"], s["repetition_penalty"]] for s in rows], dtype=torch.float32)
    t.view(torch.int32)[:, 0] = torch.tensor([s["top_k"] for s in rows], dtype=torch.int32)
    return t.view(torch.int32).to(gpu)


def _case(gpu, injected=True, idx=(0, 3, 12, 5), ylen=(4, 5, 3, 6), status=(RUNNING,) * 4, nforce=(0,) * 4,
          limit=(100,) * 4, sets=(SET_A,) * 4, seed=5):
    """B = 4 rows with their own counters; y holds ycount = ylen + idx random tokens per row, -1 behind them"""
    from easevoice_trainer_amd.hip import lib as L

    g = torch.Generator().manual_seed(seed)
    ycount = [ylen[b] + idx[b] for b in range(B)]
    logits = torch.randn(3, B, V, generator=g) * 3              # one set per consecutive step
    y = torch.full((B, YMAX), -1, dtype=torch.int64)
    for b in range(B):
        y[b, :ycount[b]] = torch.randint(0, 1024, (ycount[b],), generator=g)
    noise = torch.empty(32, B, V).exponential_(1, generator=g) if injected else None
    rstate = [[50 + ycount[b], idx[b], ycount[b], ylen[b], limit[b], status[b], (b + 1) % B, nforce[b]] for b in range(B)]
    return SimpleNamespace(L=L, idx=list(idx), ylen=list(ylen), ycount=ycount, status=list(status), logits=logits, y=y,
                           noise=noise, rstate=rstate, sets=list(sets), cols=[(b + 1) % B for b in range(B)],
                           emb=torch.randn(V, E, generator=g), pe=torch.randn(NPOS, E, generator=g),
                           alpha=torch.tensor([0.7]), row_seed=[[0x1234567 + 7 * b, b % 3] for b in range(B)],
                           sp=L.SampleParams(V, EOS, 2, 1, YMAX, 0.3, 5.0, 3.0, 123, B if injected else 1))


def _dev(t, gpu):
    """the read-only device arrays of a case"""
    return SimpleNamespace(logits=t.logits.to(gpu), noise=None if t.noise is None else t.noise.to(gpu), emb=t.emb.to(gpu),
                           pe=t.pe.to(gpu), alpha=t.alpha.to(gpu), row_seed=_i32(t.row_seed, gpu),
                           table=_table(t.sets, gpu))


def _state(t, gpu):
    return dict(rstate=_i32(t.rstate, gpu), y=t.y.to(gpu), stop=torch.full((B,), -1, dtype=torch.int32, device=gpu),
                probs=torch.full((B, V), FILL, device=gpu), x=torch.full((B, E), FILL, device=gpu),
                logp=torch.full((B, YMAX, 2), FILL, device=gpu))


def _launch(t, d, s, which, step=0, logp=True):
    """which: "f", "lp" or "p"; the values of p's four sampling fields are junk, the table decides"""
    L = t.L
    head = (C.byref(t.sp), L.ptr(d.table), L.ptr(d.logits[step]), L.ptr(s["y"]), L.ptr(s["rstate"]), L.ptr(d.noise),
            L.ptr(s["stop"]), L.ptr(s["probs"]), L.ptr(d.row_seed), None, L.ptr(d.emb), L.ptr(d.pe), L.ptr(d.alpha),
            C.c_float(1.3), L.ptr(s["x"]))
    tail = (B, E, NPOS, 1, L.stream_ptr())
    lib = L.lib()
    if which == "f":
        L.check(lib.evt_dec_sample_embed_rows_f(*head, L.ptr(s["logp"]) if logp else None, *tail), "rows_f")
    elif which == "lp":
        L.check(lib.evt_dec_sample_embed_rows_lp(*head, L.ptr(s["logp"]), *tail), "rows_lp")
    else:
        L.check(lib.evt_dec_sample_embed_rows_p(*head, *tail), "rows_p")
    torch.cuda.synchronize()


@pytest.mark.parametrize("injected", [False, True], ids=["builtin_noise", "noise_table"])
def test_unforced_rows_equal_the_lp_and_p_kernels_bit_for_bit(gpu, injected):
    """nforce = 0 in every row (one row idle): over three consecutive steps y, rstate, stop, x, probabilities and logp of
    evt_dec_sample_embed_rows_f equal those of evt_dec_sample_embed_rows_lp, and with row_logp = NULL those of
    evt_dec_sample_embed_rows_p (logp untouched), torch.equal after every launch"""
    t = _case(gpu, injected, status=(RUNNING, RUNNING, RUNNING, IDLE))
    d = _dev(t, gpu)
    f_lp, lp, f_p, p = (_state(t, gpu) for _ in range(4))
    for step in range(3):
        _launch(t, d, f_lp, "f", step)
        _launch(t, d, lp, "lp", step)
        _launch(t, d, f_p, "f", step, logp=False)
        _launch(t, d, p, "p", step)
        for name in NAMES:
            assert torch.equal(f_lp[name], lp[name]), (step, name)
            assert torch.equal(f_p[name], p[name]), (step, name)
        assert torch.equal(f_p["y"], f_lp["y"]) and bool((f_p["logp"] == FILL).all())
    st = f_lp["rstate"].tolist()
    assert [st[b][1] for b in range(3)] == [t.idx[b] + 3 for b in range(3)] and st[3] == t.rstate[3]
    assert int((f_lp["logp"] != FILL).sum()) == 3 * 3 * 2


def _oracle(t, b, step=0):
    """float64 references of row b: (log_softmax of the raw logits over Ve, the sampler's probabilities)"""
    from oracle.s1_step import logits_to_probs

    Ve = V - 1 if t.idx[b] < 1 else V
    s = t.sets[b]
    raw = t.logits[step, b:b + 1, :Ve]
    pr = logits_to_probs(raw.clone(), t.y[b:b + 1, :t.ycount[b]], s["temperature"], s["top_k"] if s["top_k"] > 0 else None,
                         s["top_p"], s["repetition_penalty"])
    return torch.log_softmax(raw[0].double(), -1), pr[0].double()


def test_mixed_rows_in_one_launch(gpu):
    """row 0 unforced, row 1 with 2 of its 3 forced steps left, row 2 forced to EOS at this step, row 3 idle; the noise
    table would make every forced row draw ANOTHER token (1e-30 at another column: the lp kernel on the same state draws
    it).  The forced tokens land in y, row 2 stops with STOP_EOS and stop = idx, row 3 is untouched, row 0 is the lp
    kernel's row; logp[..][0] within 1e-4 of a float64 log_softmax at the forced token and logp[..][1] within 1e-4 of
    the float64 log of the oracle sampler's probability (the bound of test_lp_sampler_values against float64: an fp32
    sum of 1025 terms carries at most about 6e-5 into log(sum)).  And a forced step is, bit for bit, the sampled step
    that drew the same token: the lp kernel with 1e-30 planted at the forced tokens gives the same y, rstate, stop, x
    and logp"""
    t = _case(gpu, True, idx=(2, 1, 3, 4), nforce=(0, 3, 4, 2), status=(RUNNING, RUNNING, RUNNING, IDLE))
    given, other = {1: 77, 2: EOS}, {1: 500, 2: 321}
    for b, tok in given.items():
        t.y[b, t.ycount[b]] = tok
        t.noise[t.idx[b], t.cols[b], other[b]] = 1e-30
    d = _dev(t, gpu)
    got, drawn = _state(t, gpu), _state(t, gpu)
    _launch(t, d, got, "f")
    _launch(t, d, drawn, "lp")
    yd = drawn["y"].tolist()
    assert all(yd[b][t.ycount[b]] == other[b] for b in given)              # the draw really is another token
    y, st, stop = got["y"].tolist(), got["rstate"].tolist(), got["stop"].tolist()
    assert y[1][t.ycount[1]] == 77 and y[2][t.ycount[2]] == EOS
    assert st[1] == [t.rstate[1][0] + 1, 2, t.ycount[1] + 1, t.ylen[1], 100, RUNNING, t.cols[1], 3] and stop[1] == -1
    assert st[2][5] == STOP_EOS and stop[2] == t.idx[2] and st[2][:5] == t.rstate[2][:5]
    assert st[3] == t.rstate[3] and stop[3] == -1 and torch.equal(got["y"][3].cpu(), t.y[3])
    assert bool((got["x"][3] == FILL).all()) and bool((got["logp"][3] == FILL).all())
    for name in NAMES:                                                     # row 0: nothing forced
        assert torch.equal(got[name][0], drawn[name][0]), name
    lp = got["logp"].cpu()
    worst = [0.0, 0.0]
    for b, tok in given.items():
        want0, pr = _oracle(t, b)
        assert float(pr[tok]) > 0
        g0, g1 = float(lp[b, t.ycount[b], 0]), float(lp[b, t.ycount[b], 1])
        worst = [max(worst[0], abs(g0 - float(want0[tok]))), max(worst[1], abs(g1 - float(torch.log(pr[tok]))))]
    print("max |row_logp - float64 reference| of the forced steps (model, sampler):", worst)
    assert worst[0] <= 1e-4 and worst[1] <= 1e-4, worst
    # ---- the sampled step that draws the given tokens ----
    for b, tok in given.items():
        t.noise[t.idx[b], t.cols[b], other[b]] = 1.0
        t.noise[t.idx[b], t.cols[b], tok] = 1e-30
    d2 = _dev(t, gpu)
    same = _state(t, gpu)
    _launch(t, d2, same, "lp")
    for name in ("y", "rstate", "stop", "x", "logp"):
        for b in given:
            assert torch.equal(got[name][b], same[name][b]), (name, b)


def test_a_token_the_sampler_cut(gpu):
    """top_k = 5 and a forced token outside the five largest logits: logp[..][1] is -inf, [0] is finite and within 1e-4
    of float64, the token is appended and embedded (x = emb[token] * x_scale + alpha * pe[ylen + idx]) and the row moves"""
    cut = dict(top_k=5, top_p=1.0, temperature=0.7, repetition_penalty=1.35)
    t = _case(gpu, True, idx=(2, 1, 3, 4), nforce=(0, 2, 0, 0), sets=(SET_A, cut, SET_A, SET_A))
    b = 1
    tok = int(torch.argmin(t.logits[0, b, :EOS]))
    t.y[b, t.ycount[b]] = tok
    want0, pr = _oracle(t, b)
    assert float(pr[tok]) == 0.0
    d = _dev(t, gpu)
    got = _state(t, gpu)
    _launch(t, d, got, "f")
    lp = got["logp"][b, t.ycount[b]].tolist()
    assert lp[1] == float("-inf") and abs(lp[0] - float(want0[tok])) <= 1e-4, lp
    assert float(got["probs"][b, tok]) == 0.0
    assert int(got["y"][b, t.ycount[b]]) == tok and got["rstate"][b].tolist()[1:3] == [t.idx[b] + 1, t.ycount[b] + 1]
    x = t.emb[tok].double() * float(torch.tensor(1.3, dtype=torch.float32)) + 0.7 * t.pe[t.ylen[b] + t.idx[b]].double()
    assert torch.allclose(got["x"][b].cpu().double(), x, rtol=1e-6, atol=1e-6)


def test_argmax_rule_is_off_in_forced_steps_and_on_after_them(gpu):
    """logits whose penalised arg-max is EOS in every row (idx >= 1, so the column is there).  Row 0 (nforce > idx) keeps
    running with its forced token; row 1 (nforce == idx: the first sampled step) and row 2 (nforce = 0) stop with
    STOP_EOS as ever; row 3 is forced at the last step of its limit and stops with STOP_LIMIT"""
    t = _case(gpu, True, idx=(2, 3, 3, 4), nforce=(3, 3, 0, 9), limit=(100, 100, 100, 5))
    t.logits[:, :, EOS] = 40.0
    t.y[0, t.ycount[0]] = 7
    t.y[3, t.ycount[3]] = 9
    d = _dev(t, gpu)
    got = _state(t, gpu)
    _launch(t, d, got, "f")
    st, stop, y = got["rstate"].tolist(), got["stop"].tolist(), got["y"].tolist()
    assert st[0][5] == RUNNING and st[0][1] == 3 and y[0][t.ycount[0]] == 7 and stop[0] == -1
    assert st[1][5] == STOP_EOS and stop[1] == 3 and st[2][5] == STOP_EOS and stop[2] == 3
    assert st[3][5] == STOP_LIMIT and stop[3] == 4 and y[3][t.ycount[3]] == 9
    assert torch.isfinite(got["logp"][0, t.ycount[0]]).all()


def test_an_out_of_range_forced_token_stays_inside_the_tables(gpu):
    """the host validates forced tokens; the kernel still keeps a bad value in y away from the embedding table and the
    logits: it is stored as the all-NaN marker 0x7fffffff, embeds row 0 and reports NaN log-probabilities"""
    t = _case(gpu, True, idx=(2, 1, 3, 4), nforce=(3, 2, 0, 0))
    t.y[0, t.ycount[0]] = V
    t.y[1, t.ycount[1]] = -5
    d = _dev(t, gpu)
    got = _state(t, gpu)
    _launch(t, d, got, "f")
    for b in (0, 1):
        assert int(got["y"][b, t.ycount[b]]) == 0x7FFFFFFF and bool(torch.isnan(got["logp"][b, t.ycount[b]]).all())
        x = t.emb[0].double() * float(torch.tensor(1.3, dtype=torch.float32)) + 0.7 * t.pe[t.ylen[b] + t.idx[b]].double()
        assert torch.allclose(got["x"][b].cpu().double(), x, rtol=1e-6, atol=1e-6)


# ---- sessions ----
@pytest.fixture(scope="module")
def model(gpu):
    from easevoice_trainer_amd.train.s1_engine import S1Engine

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "gpt.yaml")))
    eng = S1Engine(cfg, gpu, torch.float32)
    fill_module(eng.model, 3)
    eng.model.eval()
    return eng.model


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(HERE, "golden", "s1_logprobs.pt"), weights_only=False)


@pytest.fixture(scope="module")
def inputs(gold):
    from make_golden_s1_rows import rows_inputs

    return rows_inputs(gold["texts"] * gold["candidates"])


GRAPH = pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "eager"])


@pytest.mark.parametrize("name", ["A", "D"])
@GRAPH
def test_resume_from_forced_prefix_on_the_kernels(gpu, model, gold, inputs, graph, name, monkeypatch):
    """12 requests through 5 slots, request j forced over the first k_j of its golden tokens (0, 1, half, all, all + EOS):
    y and idx are the fixture's exactly; every log-probability, forced step or sampled, within LP_TOL_GPU = 1.526e-5 (the
    bound of test_s1_stream_candidates_gpu.py for this fixture; the measured maximum is printed before the assertion)"""
    monkeypatch.setenv("EVT_DECODE_GRAPH", graph)
    outs = resume_case(model, inputs, gold, name, gpu)
    st = model._infer().stream_stats
    if graph == "0":
        assert st["graph_captured"] is False
    assert st["admissions"] > 1
    check_rows(outs, gold["sets"][name], LP_TOL_GPU, note=f" resume set {name} gpu graph={graph}")


@GRAPH
def test_score_stream_under_junk_noise_on_the_kernels(gpu, model, gold, inputs, graph, monkeypatch):
    monkeypatch.setenv("EVT_DECODE_GRAPH", graph)
    check_scores(score_case(model, inputs, gold, gpu), LP_TOL_GPU, f" set A gpu graph={graph}")


@GRAPH
def test_preempt_and_resume_on_the_kernels(gpu, model, gold, inputs, graph, monkeypatch):
    monkeypatch.setenv("EVT_DECODE_GRAPH", graph)
    first, st, second = preempt_case(model, inputs, gold, gpu)
    check_preempt(first, st, second, gold["sets"]["A"], LP_TOL_GPU, note=f" gpu graph={graph}")


def test_a_stream_without_the_new_keys_launches_what_it_did(gpu, model, gold, inputs, monkeypatch):
    """6 slots (no other test's session), library calls counted through a wrapper on L.lib(): two plain streams never
    call evt_dec_sample_embed_rows_f and the second replays the graph the first captured (the old key); a stream with a
    forced request calls it, at step 0 and in a capture of its own, and yields the same tokens"""
    from easevoice_trainer_amd.hip import lib as L

    monkeypatch.setenv("EVT_DECODE_GRAPH", "1")
    real, calls = L.lib, {}

    class Counted:
        def __getattr__(self, name):
            calls[name] = calls.get(name, 0) + 1
            return getattr(real(), name)

    monkeypatch.setattr(L, "lib", lambda: Counted())
    g = gold["sets"]["A"]
    # the table is on the device already, so every stream passes the same pointer into the graph key
    kw = dict(slots=6, noise=inputs["q"].to(gpu), early_stop_num=gold["early_stop_num"], **g["args"])
    runs = []
    for _ in range(2):
        runs.append(list(model.decode_stream(row_requests(inputs, range(12), gpu), **kw)))
        runs.append(model._infer().stream_stats["graph_captured"])
    assert calls.get("evt_dec_sample_embed_rows_f", 0) == 0 and calls.get("evt_dec_sample_embed_rows_p", 0) > 0
    assert runs[3] is False
    check_rows(runs[0], g, 0.0)
    check_rows(runs[2], g, 0.0)
    forced = list(model.decode_stream(row_requests(inputs, range(12), gpu, {0: dict(force=g["y"][0][P:P + 2].long())}), **kw))
    assert model._infer().stream_stats["graph_captured"] is True
    assert calls.get("evt_dec_sample_embed_rows_f", 0) >= 3          # step 0, warm-up, capture
    check_rows(forced, g, 0.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_a_request_seed_reproduces_a_request_of_another_stream(gpu, model, inputs, dtype):
    """a stream seeded S decodes six requests with n = 2; an unseeded stream that holds request 5's text alone, at index
    0, with {"seed": (S + 4, 1)} yields request 5's tokens for both candidates (candidate c adds 4c to the lane), and
    with n = 1 and logprobs=False the tokens of candidate 0; an int seed s is the pair (s, 0)"""
    S = 4242
    kw = dict(top_k=15, top_p=1, early_stop_num=12, slots=7, max_text_len=24, max_prompt_len=P)
    order = [0, 1, 2, 3, 0, 2]
    reqs = row_requests(inputs, [3 * k for k in order], gpu)
    model.cd = dtype
    try:
        a = {(o.request, o.candidate): o for o in model.decode_stream(reqs, n=2, seed=S, **kw)}
        one = [(*reqs[5], dict(seed=(S + 4, 1)))]
        b = {o.candidate: o for o in model.decode_stream(one, n=2, **kw)}
        c = list(model.decode_stream(one, **kw))
        e = list(model.decode_stream([(*reqs[4], dict(seed=(S + 4, 0)))], **kw))
        f = list(model.decode_stream([(*reqs[4], dict(seed=S + 4))], **kw))
    finally:
        model.cd = torch.float32
    assert sorted(a) == [(r, k) for r in range(6) for k in range(2)] and sorted(b) == [0, 1]
    for k in (0, 1):
        assert b[k].idx == a[5, k].idx and torch.equal(b[k].y, a[5, k].y), k
    assert not torch.equal(a[5, 0].y, a[5, 1].y)
    assert len(c) == 1 and c[0][0] == 0 and c[0][2] == a[5, 0].idx and torch.equal(c[0][1], a[5, 0].y)
    assert e[0][2] == f[0][2] == a[4, 0].idx and torch.equal(e[0][1], a[4, 0].y) and torch.equal(f[0][1], a[4, 0].y)
    assert not torch.equal(a[4, 0].y, a[0, 0].y)           # the same text under another seed group

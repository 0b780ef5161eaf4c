"""GPU: per-request sampling parameters and cancellation in a refilled s1 decode session.  The row-table sampler
(evt_dec_sample_embed_rows_p, csrc/s1_decode_stream.hip) against masked launches of the session-wide entry point, bit for
bit; mixed sessions against the reference's token lists (tests/golden/s1_mixed_sampling.pt, fp32) and against
infer_panel_batch_infer under a seed; one captured graph for two parameter sets; cancellation under graph replay; bf16
repeatability; the fragment pipeline with per-fragment values and a cancelled fragment."""
import ctypes as C
import json
import os
import sys

import pytest
import torch
import yaml

from test_s1_stream_gpu import _batch, _i32, _sample_case
from test_s1_stream_sampling_cpu import _expect, _requests, cancel_scenario, check_cancel
from util_fill import fill_module

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

IDLE, RUNNING = 0, 1
SETS = [dict(top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35),
        dict(top_k=5, top_p=1, temperature=0.7, repetition_penalty=1.35),
        dict(top_k=-100, top_p=0.8, temperature=1.0, repetition_penalty=1.0),
        dict(top_k=15, top_p=0.9, temperature=1.3, repetition_penalty=1.2)]


def _table(rows, gpu):
    """evt_row_sample [B] from a list of parameter dicts"""
    t = torch.tensor([[0.0, s["top_p"], s["temperature"], s["repetition_penalty"]] for s in rows], dtype=torch.float32)
    t.view(torch.int32)[:, 0] = torch.tensor([s["top_k"] for s in rows], dtype=torch.int32)
    return t.view(torch.int32).to(gpu)


def _state(t, gpu):
    B = t.B
    return dict(rstate=_i32(t.rstate, gpu), y=t.y.to(gpu), stop=torch.full((B,), -1, dtype=torch.int32, device=gpu),
                probs=torch.full((B, t.V), -7.0, device=gpu), x=torch.full((B, t.E), -7.0, device=gpu))


def _launch(t, gpu, s, sp, table=None, mask=None):
    L = t.L
    tail = (L.ptr(t.logits), L.ptr(s["y"]), L.ptr(s["rstate"]), L.ptr(t.noise), L.ptr(s["stop"]), L.ptr(s["probs"]),
            L.ptr(_i32(t.row_seed, gpu)), L.ptr(mask), L.ptr(t.emb), L.ptr(t.pe), L.ptr(t.alpha), C.c_float(1.3),
            L.ptr(s["x"]), t.B, t.E, t.npos, 1, L.stream_ptr())
    if table is None:
        L.check(L.lib().evt_dec_sample_embed_rows(C.byref(sp), *tail), "evt_dec_sample_embed_rows")
    else:
        L.check(L.lib().evt_dec_sample_embed_rows_p(C.byref(sp), L.ptr(table), *tail), "evt_dec_sample_embed_rows_p")
    torch.cuda.synchronize()


def _with(t, s):
    sp = t.L.SampleParams.from_buffer_copy(t.sp)
    sp.top_k, sp.top_p, sp.temperature, sp.repetition_penalty = (s["top_k"], s["top_p"], s["temperature"],
                                                                   s["repetition_penalty"])
    return sp


@pytest.mark.parametrize("injected", [False, True], ids=["builtin_noise", "noise_table"])
def test_row_table_sampler_equals_masked_launches(gpu, injected):
    """B = 12, V = 1025, E = 512 (one row idle, one at its limit, one with EOS by arg-max), the rows taking sets A-D in
    turn: one launch with the table gives, bit for bit, y / rstate / stop / x / probabilities of four launches of the
    session-wide entry point, each with one set in p and a mask of that set's rows; the values in p are then ignored;
    and a table filled with p's own values is the session-wide entry point over all rows"""
    t = _sample_case(gpu, injected)
    B = t.B
    got = _state(t, gpu)
    junk = _with(t, dict(top_k=2, top_p=0.3, temperature=5.0, repetition_penalty=3.0))     # must not be read
    _launch(t, gpu, got, junk, table=_table([SETS[b % 4] for b in range(B)], gpu))
    ref = _state(t, gpu)
    for k, s in enumerate(SETS):
        _launch(t, gpu, ref, _with(t, s), mask=_i32([1 if b % 4 == k else 0 for b in range(B)], gpu))
    for name in ("y", "rstate", "stop", "x", "probs"):
        assert torch.equal(got[name], ref[name]), name
    toks = [int(got["y"][b, t.ycount[b]]) for b in range(B)]
    assert toks[11] == -1 and all(0 <= v <= 1024 for v in toks[:11])
    nz = (got["probs"][:11] > 0).sum(1).tolist()
    assert nz[1] <= 5 and nz[3] <= 15 and nz[4] > 100 and 1 <= nz[2] < 1024, nz    # the sets really differ per row
    # ---- uniform table == session-wide entry point ----
    own = dict(top_k=t.sp.top_k, top_p=t.sp.top_p, temperature=t.sp.temperature,
               repetition_penalty=t.sp.repetition_penalty)
    a, b_ = _state(t, gpu), _state(t, gpu)
    _launch(t, gpu, a, junk, table=_table([own] * B, gpu))
    _launch(t, gpu, b_, t.sp)
    for name in ("y", "rstate", "stop", "x", "probs"):
        assert torch.equal(a[name], b_[name]), name


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
    return torch.load(os.path.join(HERE, "golden", "s1_mixed_sampling.pt"), weights_only=False)


def _dev(d, gpu):
    return dict(d, x=[v.to(gpu) for v in d["x"]], bert=[v.to(gpu) for v in d["bert"]], prompts=d["prompts"].to(gpu))


@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "eager"])
def test_mixed_sets_match_reference_tokens(gpu, model, gold, graph, monkeypatch):
    """twelve requests with sets r % 4 through 5 slots, fp32: the reference's tokens and indices, request for request"""
    from make_golden_s1_rows import rows_inputs

    monkeypatch.setenv("EVT_DECODE_GRAPH", graph)
    R = gold["R"]
    d = _dev(rows_inputs(R), gpu)
    out = {r: (y, i) for r, y, i in model.decode_stream(_requests(d, gold, range(R)), slots=5, noise=d["q"], top_k=3,
                                                        top_p=0.5, temperature=2.0, repetition_penalty=1.1,
                                                        early_stop_num=gold["early_stop_num"])}
    st = model._infer().stream_stats
    assert sorted(out) == list(range(R)) and st["admissions"] >= 3
    if graph == "0":
        assert st["graph_captured"] is False
    bad = []
    for r in range(R):
        y, idx = _expect(gold, r)
        if out[r][1] != idx or not torch.equal(out[r][0].cpu().long(), y):
            bad.append((r, out[r][1], idx))
    assert not bad, bad


def test_mixed_sets_match_uniform_runs_under_a_seed(gpu, model):
    """ten requests with sets r % 4 under seed 4242 through 5 slots: request r's tokens are those of
    infer_panel_batch_infer(seed=4242, **set) on the same ten texts, compared on that set's members (every group of
    four holds the longest text, so the key positions agree)"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(20)
    order = [0, 3, 5, 7, 0, 2, 4, 6, 0, 1]
    dd = _dev(d, gpu)
    reqs = [(dd["x"][t], dd["bert"][t], dd["prompts"][t], SETS[r % 4]) for r, t in enumerate(order)]
    got = {r: (y, i) for r, y, i in model.decode_stream(reqs, slots=5, seed=4242, early_stop_num=12)}
    assert model._infer().stream_stats["admissions"] >= 2
    for k, s in enumerate(SETS):
        ys, idxs = _batch(model, gpu, d, order, seed=4242, early_stop_num=12, **s)
        for r in range(k, len(order), 4):
            assert got[r][1] == idxs[r], (r, got[r][1], idxs[r])
            assert torch.equal(got[r][0], ys[r]), r
    assert not torch.equal(got[0][0], got[4][0])


def test_one_graph_serves_every_parameter_set(gpu, model):
    """two streams of one capacity (7 slots: no other test's session) under seed 4242, set A then set B session-wide:
    the first captures, the second replays that graph and still samples with its own values"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(20)
    order = [0, 3, 5, 7, 0, 2, 4, 6, 0, 1]
    dd = _dev(d, gpu)
    reqs = [(dd["x"][t], dd["bert"][t], dd["prompts"][t]) for t in order]
    outs = []
    for s, captured in ((SETS[0], True), (SETS[1], False)):
        got = {r: (y, i) for r, y, i in model.decode_stream(reqs, slots=7, seed=4242, early_stop_num=12, **s)}
        assert model._infer().stream_stats["graph_captured"] is captured
        ys, idxs = _batch(model, gpu, d, order, seed=4242, early_stop_num=12, **s)
        for r in range(len(order)):
            assert got[r][1] == idxs[r] and torch.equal(got[r][0], ys[r]), (s, r)
        outs.append(got)
    assert any(not torch.equal(outs[0][r][0], outs[1][r][0]) for r in range(len(order)))


def _session(model):
    inf = model._infer()
    return inf._sessions[inf._wide[-1]]


def test_cancel_under_graph_replay(gpu, model, gold, monkeypatch):
    """the CPU tier's cancel scenario on the kernels with graph replay; then a stream whose cancelled slot is not
    refilled: its status is IDLE at the cancel poll, and its counters and its y row at the end of the stream are those
    of the cancel poll although another row went on for ten more replays"""
    from make_golden_s1_rows import rows_inputs
    from easevoice_trainer_amd.auto_reg.t2s_infer import StreamControl

    monkeypatch.setenv("EVT_DECODE_GRAPH", "1")
    d = rows_inputs(gold["R"])
    check_cancel(*cancel_scenario(model, d, gold, dev=gpu))
    rows = [11, 0, 1]                            # request 0 stops at step 1; 1 and 2 live to the early stop
    reqs = [(d["x"][r].to(gpu), d["bert"][r].to(gpu), d["prompts"][r].to(gpu)) for r in rows]
    a = dict(gold["sets"][0]["args"], early_stop_num=gold["early_stop_num"], slots=3, poll=1)
    ctl, got, snap = StreamControl(), [], {}
    for item in model.decode_stream(reqs, noise=d["q"][:, rows].contiguous().to(gpu), control=ctl, **a):
        got.append(item)
        if len(got) == 1:
            assert item[0] == 0
            ctl.cancel(1)
        elif item[1] is None:
            S = _session(model)
            torch.cuda.synchronize()
            snap = dict(rstate=S.rstate[1].clone(), y=S.y[1].clone(), steps=model._infer().stream_stats["steps"])
    st = model._infer().stream_stats
    assert st["graph_captured"] in (True, False) and [r for r, _y, _i in got] == [0, 1, 2] and got[1][1] is None
    S = _session(model)
    torch.cuda.synchronize()
    assert int(snap["rstate"][5]) == IDLE and int(snap["rstate"][1]) == snap["steps"] + 1 < 5    # step 0 + the replays
    assert st["steps"] >= snap["steps"] + 10
    assert torch.equal(S.rstate[1], snap["rstate"]) and torch.equal(S.y[1], snap["y"])
    assert int((S.y[1, 12:] != 0).sum()) <= snap["steps"] + 1
    y2, i2 = gold["sets"][0]["y"][1].long(), gold["sets"][0]["idx"][1]
    assert got[2][2] == i2 and torch.equal(got[2][1].cpu().long(), y2)


def test_mixed_bf16_repeatable(gpu, model):
    """40 requests with sets r % 4 and their own step limits through 32 slots in bf16 under one seed: the same tokens
    twice, all of them valid, every index within the request's own limit"""
    from make_golden_s1_rows import rows_inputs

    R = 40
    d = _dev(rows_inputs(R), gpu)
    lims = [18 + 3 * (r % 5) for r in range(R)]
    per = {k: [SETS[r % 4][k] for r in range(R)] for k in SETS[0]}
    model.cd = torch.bfloat16
    try:
        out = [model.infer_panel_batch_infer_refill(d["x"], d["x_lens"], d["prompts"], d["bert"], slots=32, seed=77,
                                                    early_stop_num=lims, **per) for _ in range(2)]
        adm = model._infer().stream_stats["admitted"]
    finally:
        model.cd = torch.float32
    (ys1, i1), (ys2, i2) = out
    assert i1 == i2 and len(ys1) == R and adm[0] == 32 and sum(adm) == R
    assert all(torch.equal(a, b) for a, b in zip(ys1, ys2))
    for r, (y, i) in enumerate(zip(ys1, i1)):
        assert 0 <= i <= lims[r] and int(y.min()) >= 0 and int(y[12:].max()) <= 1024 and y.numel() > 12, (r, i)
        assert y.numel() <= 12 + lims[r] + 1


def test_synthesize_stream_fragment_sampling_and_cancel(gpu):
    """fragment_sampling whose entries equal the session-wide values gives the waveforms of the call without it, bit
    for bit; a fragment cancelled after the first hand-out comes back as (index, None), the other is unchanged"""
    from make_golden_s1_inputs import pipeline_inputs
    from util_fill import decode_inputs
    from easevoice_trainer_amd.auto_reg.t2s_infer import StreamControl
    from easevoice_trainer_amd.auto_reg.t2s_model import Text2SemanticDecoder
    from easevoice_trainer_amd.inference.pipeline import synthesize_stream
    from easevoice_trainer_amd.inference.sovits import SoVITSVoice
    from easevoice_trainer_amd.inference.t2s import T2SVoice
    from easevoice_trainer_amd.module import models

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "gpt.yaml")))
    hps = json.load(open(os.path.join(ROOT, "configs", "s2.json")))
    d, dd = pipeline_inputs(), decode_inputs()
    src = Text2SemanticDecoder(cfg)
    fill_module(src, 3)
    t2s = T2SVoice({"weight": {"model." + k: v.clone() for k, v in src.state_dict().items()}, "config": cfg, "info": "x"},
                   device=str(gpu), dtype=torch.float32)
    net = models.SynthesizerTrn(1025, 32, n_speakers=300, **hps["model"])
    fill_module(net, 1)
    voice = SoVITSVoice({"weight": {k: v.clone() for k, v in net.state_dict().items() if "enc_q" not in k}, "config": hps,
                         "info": "x"}, device=str(gpu), dtype=torch.float32)
    wide = dict(top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35)
    kw = dict(speed_factor=1.25, decode_kwargs=dict(noise=dd["noise"].to(gpu)), sample_kwargs=dict(noise=d["q"], poll=2),
              **wide)
    args = (t2s, voice, d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], dd["refers"])
    base = list(synthesize_stream(*args, **kw))
    assert [i for i, _w in base] == [1, 0]
    same = list(synthesize_stream(*args, fragment_sampling=[dict(wide), dict(wide, early_stop_num=t2s.early_stop_num)],
                                  **kw))
    assert [i for i, _w in same] == [1, 0]
    for (_i, w0), (_j, w1) in zip(base, same):
        assert torch.equal(w0, w1)
    ctl, got = StreamControl(), []
    for item in synthesize_stream(*args, fragment_sampling=[None, dict(wide)], control=ctl, **kw):
        got.append(item)
        if len(got) == 1:
            ctl.cancel(0)
    assert [i for i, _w in got] == [1, 0] and got[1][1] is None
    assert torch.equal(got[0][1], base[0][1])
    ev = t2s.model._infer().stream_stats["events"]
    assert [(k, r) for k, _s, r, _slot in ev if k != "admit"] == [("finish", 1), ("cancel", 0)]

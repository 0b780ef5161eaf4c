"""GPU: candidates per request and per-token log-probabilities in a refilled s1 decode session.  The sampler with
log-probabilities (evt_dec_sample_embed_rows_lp, csrc/s1_decode_stream.hip) against evt_dec_sample_embed_rows_p bit for
bit and against float64 references; n = 3 sessions against the reference's tokens and log-probabilities
(tests/golden/s1_logprobs.pt, fp32), the shared prompt pass, the noise lanes under a seed, the graph key, and the
fragment pipeline with candidates."""
import ctypes as C
import json
import os
import sys

import pytest
import torch
import yaml

from test_s1_stream_candidates_cpu import check_against_fixture, requests
from test_s1_stream_gpu import _batch, _i32, _sample_case, rel
from test_s1_stream_sampling_gpu import SETS, _state, _table, _with
from util_fill import fill_module

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

IDLE, RUNNING = 0, 1
FILL = -7.0
# Bound on |log-probability - fixture| of the fp32 session: the logits of the kernels against those of the reference on
# the CPU.  Measured on an MI355X: 3.815e-6 for sets A and D alike, with graph replay and with eager launches (two ulp
# of a log-probability around -7); the bound is four times that.  One column too many or too few in the log-sum-exp
# over V = 1025 near-uniform logits moves a value by about 1e-3, far outside it.
LP_TOL_GPU = 4 * 3.815e-6


def _launch_lp(t, gpu, s, sp, table, logp, mask=None, lp=True):
    L = t.L
    head = (C.byref(sp), L.ptr(table), L.ptr(t.logits), L.ptr(s["y"]), L.ptr(s["rstate"]), L.ptr(t.noise),
            L.ptr(s["stop"]), L.ptr(s["probs"]), L.ptr(_i32(t.row_seed, gpu)), L.ptr(mask), L.ptr(t.emb), L.ptr(t.pe),
            L.ptr(t.alpha), C.c_float(1.3), L.ptr(s["x"]))
    tail = (t.B, t.E, t.npos, 1, L.stream_ptr())
    if lp:
        L.check(L.lib().evt_dec_sample_embed_rows_lp(*head, L.ptr(logp), *tail), "evt_dec_sample_embed_rows_lp")
    else:
        L.check(L.lib().evt_dec_sample_embed_rows_p(*head, *tail), "evt_dec_sample_embed_rows_p")
    torch.cuda.synchronize()


def _written(logp):
    """(row, position) pairs of a [B][ymax][2] buffer that no longer hold the fill value"""
    return sorted(set((int(b), int(j)) for b, j, _k in (logp != FILL).nonzero().tolist()))


@pytest.mark.parametrize("injected", [False, True], ids=["builtin_noise", "noise_table"])
def test_lp_sampler_equals_row_table_sampler_bit_for_bit(gpu, injected):
    """B = 12, V = 1025, E = 512 (one row idle, one at its limit, one with EOS by arg-max), the rows taking sets A-D in
    turn: one launch with log-probabilities gives y / rstate / stop / x / probabilities torch.equal to one launch of
    evt_dec_sample_embed_rows_p, and writes row_logp at [b][ycount] of the rows that ran and nowhere else; a second
    launch writes at ycount + 1 for the rows that moved and nowhere for the rows that stopped; a masked launch writes
    for the chosen rows only; a null row_logp is refused"""
    t = _sample_case(gpu, injected)
    B, L = t.B, t.L
    table = _table([SETS[b % 4] for b in range(B)], gpu)
    junk = _with(t, dict(top_k=2, top_p=0.3, temperature=5.0, repetition_penalty=3.0))
    got, ref = _state(t, gpu), _state(t, gpu)
    logp = torch.full((B, t.ymax, 2), FILL, device=gpu)
    _launch_lp(t, gpu, got, junk, table, logp)
    _launch_lp(t, gpu, ref, junk, table, None, lp=False)
    for name in ("y", "rstate", "stop", "x", "probs"):
        assert torch.equal(got[name], ref[name]), name
    ran = [b for b in range(B) if t.status[b] == RUNNING]
    assert _written(logp) == [(b, t.ycount[b]) for b in ran] and 11 not in ran
    first = logp.clone()
    assert torch.isfinite(first[ran, [t.ycount[b] for b in ran]]).all()
    # ---- second launch ----
    st = got["rstate"].tolist()
    moved = [b for b in ran if st[b][5] == RUNNING]
    assert 3 not in moved and 5 not in moved and len(moved) >= 8       # the row at its limit and the EOS row stopped
    _launch_lp(t, gpu, got, junk, table, logp)
    _launch_lp(t, gpu, ref, junk, table, None, lp=False)
    for name in ("y", "rstate", "stop", "x", "probs"):
        assert torch.equal(got[name], ref[name]), name
    assert _written(logp) == sorted([(b, t.ycount[b]) for b in ran] + [(b, t.ycount[b] + 1) for b in moved])
    assert all(torch.equal(logp[b, t.ycount[b]], first[b, t.ycount[b]]) for b in ran)
    # ---- masked launch (step 0 of an admission) ----
    chosen = [1, 4, 11]                                          # 11 is idle: chosen, but still skipped
    ms, lpm = _state(t, gpu), torch.full((B, t.ymax, 2), FILL, device=gpu)
    _launch_lp(t, gpu, ms, junk, table, lpm, mask=_i32([1 if b in chosen else 0 for b in range(B)], gpu))
    assert _written(lpm) == [(1, t.ycount[1]), (4, t.ycount[4])]
    assert torch.equal(lpm[1, t.ycount[1]], first[1, t.ycount[1]]) and torch.equal(lpm[4, t.ycount[4]], first[4, t.ycount[4]])
    # ---- validation ----
    s = _state(t, gpu)
    rc = L.lib().evt_dec_sample_embed_rows_lp(
        C.byref(junk), L.ptr(table), L.ptr(t.logits), L.ptr(s["y"]), L.ptr(s["rstate"]), L.ptr(t.noise), L.ptr(s["stop"]),
        None, L.ptr(_i32(t.row_seed, gpu)), None, L.ptr(t.emb), L.ptr(t.pe), L.ptr(t.alpha), C.c_float(1.3), L.ptr(s["x"]),
        None, t.B, t.E, t.npos, 1, L.stream_ptr())
    assert rc != 0


@pytest.mark.parametrize("injected", [False, True], ids=["builtin_noise", "noise_table"])
def test_lp_sampler_values(gpu, injected):
    """row_logp[..., 0] against the float64 log_softmax of the same fp32 logits over the Ve columns of the row's step
    (V - 1 at step 0), row_logp[..., 1] against the float64 log of the oracle's probabilities under the row's set, both
    at the drawn token: absolute error <= 1e-4.  An fp32 sum of 1025 terms carries at most about 1025 * 2^-24 = 6e-5
    relative error into log(sum); the subtraction of the maximum adds a few ulp of |logit| <= 64, below 1e-5.  The
    sampler's value is finite for every drawn token (it has a probability > 0 in probs_out) and is the log of that
    probability"""
    from oracle.s1_step import logits_to_probs

    t = _sample_case(gpu, injected)
    B = t.B
    sets = [SETS[b % 4] for b in range(B)]
    got = _state(t, gpu)
    logp = torch.full((B, t.ymax, 2), FILL, device=gpu)
    _launch_lp(t, gpu, got, _with(t, SETS[0]), _table(sets, gpu), logp)
    logits, y, probs, lp = t.logits.cpu(), t.y, got["probs"].cpu(), logp.cpu()
    worst = [0.0, 0.0]
    for b in range(B):
        if t.status[b] != RUNNING:
            continue
        Ve = t.V - 1 if t.idx[b] < 1 else t.V
        tok = int(got["y"][b, t.ycount[b]])
        assert 0 <= tok < Ve
        want0 = torch.log_softmax(logits[b, :Ve].double(), -1)[tok]
        s = sets[b]
        pr = logits_to_probs(logits[b:b + 1, :Ve], y[b:b + 1, :t.ycount[b]], s["temperature"],
                             s["top_k"] if s["top_k"] > 0 else None, s["top_p"], s["repetition_penalty"])
        assert float(pr[0, tok]) > 0 and float(probs[b, tok]) > 0
        assert torch.equal(probs[b, :Ve] > 0, pr[0] > 0)           # -inf exactly where the oracle's probability is 0
        want1 = torch.log(pr[0, tok].double())
        g0, g1 = float(lp[b, t.ycount[b], 0]), float(lp[b, t.ycount[b], 1])
        assert g1 > float("-inf") and g0 <= 0 and g1 <= 1e-6
        worst = [max(worst[0], abs(g0 - float(want0))), max(worst[1], abs(g1 - float(want1)))]
        assert abs(g1 - float(torch.log(probs[b, tok].double()))) <= 1e-5, b
    print("max |row_logp - float64 reference| (model, sampler):", worst)
    assert worst[0] <= 1e-4 and worst[1] <= 1e-4, worst


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

    d = rows_inputs(gold["texts"] * gold["candidates"])
    d["q4"] = d["q"].view(d["q"].size(0), gold["texts"], gold["candidates"], -1)
    return d


def _session(model):
    inf = model._infer()
    return inf._sessions[inf._wide[-1]]


@pytest.mark.parametrize("name", ["A", "D"])
@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "eager"])
def test_candidates_match_reference_on_the_kernels(gpu, model, gold, inputs, graph, name, monkeypatch):
    """the fixture's 4 x 3 candidates through 7 slots, fp32, graph replay and eager launches: tokens and indices exactly;
    log-probabilities within LP_TOL_GPU = 1.526e-5, four times the 3.815e-6 measured on an MI355X against the fixture
    (the same figure for both sets, replayed and eager; printed before the assertion).  Set D's top_k = 15 cuts the
    forced EOS, so its twelve candidates all run to the limit: stops by EOS at different steps and the staggered refill
    that follows them are checked by set A"""
    monkeypatch.setenv("EVT_DECODE_GRAPH", graph)
    g = gold["sets"][name]
    outs = list(model.decode_stream(requests(inputs, range(4), gpu), slots=7, n=3, logprobs=True, noise=inputs["q4"],
                                    early_stop_num=gold["early_stop_num"], **g["args"]))
    st = model._infer().stream_stats
    if graph == "0":
        assert st["graph_captured"] is False
    assert st["prefill_rows"][0] == 2 and st["admitted"][0] == 6 and sum(st["prefill_rows"]) == 4
    check_against_fixture(outs, gold, name, LP_TOL_GPU, dev_note=f" gpu graph={graph}")


def test_candidates_share_one_prompt_pass(gpu, model, gold, inputs):
    """12 slots: one admission with four prompt rows for twelve slots; the K and V slabs of a request's three slots are
    torch.equal over [0, Xmax + prompt_len) in every layer (the decode steps append behind that)"""
    a = gold["sets"]["A"]["args"]
    outs = list(model.decode_stream(requests(inputs, range(4), gpu), slots=12, n=3, noise=inputs["q4"],
                                    early_stop_num=gold["early_stop_num"], **a))
    st = model._infer().stream_stats
    assert st["prefill_rows"] == [4] and st["admitted"] == [12] and len(outs) == 12
    slot = {}
    for kind, _s, r, sl in st["events"]:
        if kind == "admit":
            slot.setdefault(r, []).append(sl)
    assert slot == {r: [3 * r, 3 * r + 1, 3 * r + 2] for r in range(4)}
    S = _session(model)
    n = S.Xmax + 12
    for r in range(4):
        s0 = slot[r][0]
        assert S.kc[:, s0, :n].abs().sum() > 0
        for s in slot[r][1:]:
            assert torch.equal(S.kc[:, s, :n], S.kc[:, s0, :n]) and torch.equal(S.vc[:, s, :n], S.vc[:, s0, :n]), (r, s)
    assert not torch.equal(S.kc[:, 0, :n], S.kc[:, 3, :n])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_candidate_lanes_under_a_seed(gpu, model, inputs, dtype):
    """six requests with n = 3 under seed 4242 through 7 slots: a second run gives identical tokens and bitwise identical
    log-probabilities (fp32 and bf16); candidates 1 and 2 differ from candidate 0 for at least one request; in fp32
    candidate 0 of every request has the tokens of infer_panel_batch_infer(seed=4242) text for text (one wide session on
    the same linear kernels; every group of four holds the longest text, so the key positions agree)"""
    kw = dict(top_k=15, top_p=1, early_stop_num=12)
    order = [0, 1, 2, 3, 0, 2]
    model.cd = dtype
    try:
        runs = [{(o.request, o.candidate): o for o in model.decode_stream(requests(inputs, order, gpu), slots=7, n=3,
                                                                          logprobs=True, seed=4242, **kw)}
                for _ in range(2)]
        ys, idxs = _batch(model, gpu, inputs, order, seed=4242, **kw)
    finally:
        model.cd = torch.float32
    a, b = runs
    assert sorted(a) == sorted(b) == [(r, c) for r in range(len(order)) for c in range(3)]
    for key in a:
        assert a[key].idx == b[key].idx and torch.equal(a[key].y, b[key].y), key
        assert torch.equal(a[key].logprobs, b[key].logprobs) and torch.isfinite(a[key].logprobs).all(), key
        assert a[key].logprobs.size(0) == a[key].y.numel() - 12 + 1
    if dtype == torch.float32:
        for r in range(len(order)):
            assert a[r, 0].idx == idxs[r] and torch.equal(a[r, 0].y, ys[r]), r
    for c in (1, 2):
        assert any(not torch.equal(a[r, c].y, a[r, 0].y) for r in range(len(order))), c
    assert any(not torch.equal(a[r, 1].y, a[r, 2].y) for r in range(len(order)))
    assert not torch.equal(a[0, 0].y, a[4, 0].y)          # the same text in another seed group


def test_logprobs_joins_the_graph_key(gpu, model, inputs, monkeypatch):
    """9 slots (no other test's session): a logprobs=True stream captures; a second one with other sampling values
    replays that graph; a logprobs=False stream of the same capacity does not reuse it, and yields the tokens of the
    logprobs=True stream"""
    monkeypatch.setenv("EVT_DECODE_GRAPH", "1")
    kw = dict(slots=9, n=2, seed=4242, early_stop_num=12)
    reqs = requests(inputs, range(4), gpu)
    outs = []
    for s, lp, captured in ((SETS[0], True, True), (SETS[1], True, False), (SETS[1], False, True)):
        got = {(o.request, o.candidate): o for o in model.decode_stream(reqs, logprobs=lp, **kw, **s)}
        assert model._infer().stream_stats["graph_captured"] is captured, (s, lp)
        assert all((o.logprobs is not None) == lp for o in got.values())
        outs.append(got)
    assert any(not torch.equal(outs[0][k].y, outs[1][k].y) for k in outs[0])
    for k in outs[1]:
        assert outs[1][k].idx == outs[2][k].idx and torch.equal(outs[1][k].y, outs[2][k].y), k


def test_synthesize_stream_candidates(gpu):
    """two fragments with candidates = 2: choose sees both takes of a fragment in candidate order with their
    log-probabilities, and the waveform of the chosen take equals (tolerance of test_synthesize_stream_equals_fragments)
    the candidates = 1 waveform of a stream fed that take's noise column"""
    from make_golden_s1_inputs import pipeline_inputs
    from util_fill import decode_inputs
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
    q2 = torch.empty(32, 2, 1025).exponential_(1, generator=torch.Generator().manual_seed(9))
    q2[5, 0, 1024] = 1e-30
    q2[11, 1, 1024] = 1e-30
    q4 = torch.stack([d["q"], q2], dim=2).contiguous()
    kw = dict(top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35, speed_factor=1.25,
              decode_kwargs=dict(noise=dd["noise"].to(gpu)))
    args = (t2s, voice, d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], dd["refers"])
    asked = []

    def choose(i, outs):
        asked.append((i, [o.candidate for o in outs], [None if o.logprobs is None else tuple(o.logprobs.shape) for o in outs],
                      [o.idx for o in outs]))
        return 1 - i

    got = dict(synthesize_stream(*args, candidates=2, choose=choose, sample_kwargs=dict(noise=q4, poll=2), **kw))
    assert sorted(asked) == [(0, [0, 1], [(15, 2), (6, 2)], [13, 4]), (1, [0, 1], [(10, 2), (12, 2)], [8, 10])]
    picked = torch.stack([q4[:, 0, 1], q4[:, 1, 0]], dim=1).contiguous()
    want = dict(synthesize_stream(*args, sample_kwargs=dict(noise=picked, poll=2), **kw))
    assert sorted(got) == sorted(want) == [0, 1]
    for i in (0, 1):
        assert got[i].shape == want[i].shape and rel(got[i], want[i]) < 2e-3, (i, rel(got[i], want[i]))

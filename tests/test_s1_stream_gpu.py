"""GPU: continuous batching of s1 decoding (csrc/s1_decode_stream.hip, auto_reg/t2s_infer.py StreamSession).
The two per-row kernels against the kernels with shared counters called row by row (bit for bit), the whole refilled
decode against the reference's token lists (tests/golden/s1_batch_infer_rows.pt) and against infer_panel_batch_infer
(seeded noise; two prompts of different lengths in one session), and the fragment-by-fragment pipeline."""
import ctypes as C
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import yaml

from util_fill import fill_module

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

IDLE, RUNNING, STOP_EOS, STOP_LIMIT = 0, 1, 2, 3


def _i32(v, gpu):
    return torch.tensor(v, dtype=torch.int32, device=gpu)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_dec_attn_rows_equals_one_row_calls(gpu, dtype):
    """rows at different cache positions with different text lengths: each running row's output and appended cache
    line are those of a one-row evt_dec_attn call at its position, bit for bit; idle and stopped rows leave their
    output and their cache slab untouched"""
    from easevoice_trainer_amd.hip import lib as L

    B, H, D, Lmax, x_len = 7, 16, 32, 512, 40
    E = H * D
    pos = [45, 60, 100, 300, 47, 511, 41]
    x_lens = [40, 33, 20, 40, 1, 37, 40]
    status = [RUNNING, RUNNING, RUNNING, RUNNING, IDLE, RUNNING, STOP_EOS]
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(B, 3 * E, generator=g).to(gpu)
    kc0 = torch.randn(B, Lmax, E, generator=g).to(dtype).to(gpu)
    vc0 = torch.randn(B, Lmax, E, generator=g).to(dtype).to(gpu)
    rstate = _i32([[pos[b], 3, 9, 5, 100, status[b], 0, 0] for b in range(B)], gpu)
    xl = _i32(x_lens, gpu)
    kc, vc = kc0.clone(), vc0.clone()
    out = torch.full((B, E), -7.0, device=gpu)
    L.check(L.lib().evt_dec_attn_rows(L.dt_of(kc), L.ptr(qkv), L.ptr(kc), L.ptr(vc), L.ptr(rstate), L.ptr(out), B, H, D,
                                      Lmax, L.ptr(xl), x_len, L.stream_ptr()), "evt_dec_attn_rows")
    torch.cuda.synchronize()
    kr, vr = kc0.clone(), vc0.clone()
    ref = torch.full((B, E), -7.0, device=gpu)
    for b in range(B):
        if status[b] != RUNNING:
            continue
        ctr = _i32([pos[b], 0, 0, 0, 0, 0, 0, 0], gpu)
        qb, ob, xb = qkv[b:b + 1].contiguous(), ref[b:b + 1], xl[b:b + 1].contiguous()
        L.check(L.lib().evt_dec_attn(L.dt_of(kr), L.ptr(qb), L.ptr(kr[b]), L.ptr(vr[b]), L.ptr(ctr), L.ptr(ob), 1, H, D,
                                     Lmax, L.ptr(xb), x_len, L.stream_ptr()), "evt_dec_attn")
        torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert torch.equal(kc, kr) and torch.equal(vc, vr)
    for b in range(B):
        if status[b] == RUNNING:
            assert not torch.equal(kc[b, pos[b]], kc0[b, pos[b]]) and torch.isfinite(out[b]).all()
        else:
            assert torch.equal(out[b], torch.full((E,), -7.0, device=gpu))
            assert torch.equal(kc[b], kc0[b]) and torch.equal(vc[b], vc0[b])


def _sample_case(gpu, injected):
    from easevoice_trainer_amd.hip import lib as L

    B, V, E, ymax, npos, s = 12, 1025, 512, 512, 4000, 0x1234567
    idx = [0, 3, 14, 14, 20, 5, 14, 7, 9, 30, 11, 2]
    ylen = [10 + 3 * b for b in range(B)]
    ycount = [ylen[b] + idx[b] for b in range(B)]
    limit = [100] * B
    limit[3] = idx[3] + 1                                       # this row reaches its limit in this launch
    status = [RUNNING] * B
    status[11] = IDLE
    cols = [(5 * b + 2) % B for b in range(B)]
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(B, V, generator=g) * 3)
    logits[5, 1024] = 40.0                                      # EOS by the arg-max of the logits
    logits[0, 1024] = 40.0                                      # ... but not at step 0: the EOS column is dropped there
    y = torch.full((B, ymax), -1, dtype=torch.int64)
    for b in range(B):
        y[b, :ycount[b]] = torch.randint(0, 1024, (ycount[b],), generator=g)
    emb, pe, alpha = torch.randn(V, E, generator=g), torch.randn(npos, E, generator=g), torch.tensor([0.7])
    noise = torch.empty(32, B, V).exponential_(1, generator=g).to(gpu) if injected else None
    sp = L.SampleParams(V, 1024, 15, 1, ymax, 1.0, 1.0, 1.35, 123, B if injected else 1)
    rstate = [[50 + ycount[b], idx[b], ycount[b], ylen[b], limit[b], status[b], cols[b], 0] for b in range(B)]
    row_seed = [[s + 7 * b, 0] for b in range(B)]
    t = SimpleNamespace(B=B, V=V, E=E, ymax=ymax, npos=npos, idx=idx, ylen=ylen, ycount=ycount, status=status, cols=cols,
                        logits=logits.to(gpu), y=y, emb=emb.to(gpu), pe=pe.to(gpu), alpha=alpha.to(gpu), noise=noise,
                        sp=sp, rstate=rstate, row_seed=row_seed, L=L)
    return t


def _launch_rows(t, gpu, rstate, y, stop, probs, x, mask=None, dpos=1):
    L = t.L
    L.check(L.lib().evt_dec_sample_embed_rows(
        C.byref(t.sp), L.ptr(t.logits), L.ptr(y), L.ptr(rstate), L.ptr(t.noise), L.ptr(stop), L.ptr(probs),
        L.ptr(_i32(t.row_seed, gpu)), L.ptr(mask), L.ptr(t.emb), L.ptr(t.pe), L.ptr(t.alpha), C.c_float(1.3), L.ptr(x),
        t.B, t.E, t.npos, dpos, L.stream_ptr()), "evt_dec_sample_embed_rows")
    torch.cuda.synchronize()


@pytest.mark.parametrize("injected", [False, True], ids=["builtin_noise", "noise_table"])
def test_dec_sample_embed_rows_equals_three_launches(gpu, injected):
    """12 rows with their own idx / ycount / ylen (and noise column): tokens, EOS stops, probabilities and x_next are bit
    for bit what evt_dec_sample + evt_dec_embed give when called for one row with that row's counters; the row at its
    limit and the EOS row are marked and do not move on a second launch; the counters of the others advance"""
    t = _sample_case(gpu, injected)
    L, B = t.L, t.B
    rstate, y = _i32(t.rstate, gpu), t.y.to(gpu)
    stop = torch.full((B,), -1, dtype=torch.int32, device=gpu)
    probs, x = torch.full((B, t.V), -7.0, device=gpu), torch.full((B, t.E), -7.0, device=gpu)
    _launch_rows(t, gpu, rstate, y, stop, probs, x)
    # ---- the kernels with shared counters, one row per call ----
    yr, xr, pr = t.y.to(gpu), torch.full((B, t.E), -7.0, device=gpu), torch.full((B, t.V), -7.0, device=gpu)
    sr = torch.full((B,), -1, dtype=torch.int32, device=gpu)
    sp1 = L.SampleParams(t.V, 1024, 15, 1, t.ymax, 1.0, 1.0, 1.35, 123, 1)
    for b in range(B):
        if t.status[b] != RUNNING:
            continue
        ctr = _i32([0, t.idx[b], t.ycount[b], t.ylen[b], t.row_seed[b][0], 0, 0, 0], gpu)
        nz = t.noise[:, t.cols[b]].contiguous() if injected else None
        L.check(L.lib().evt_dec_sample(C.byref(sp1), L.ptr(t.logits[b:b + 1]), L.ptr(yr[b:b + 1]), L.ptr(ctr), L.ptr(nz),
                                       L.ptr(sr[b:b + 1]), L.ptr(pr[b:b + 1]), 1, L.stream_ptr()), "evt_dec_sample")
        L.check(L.lib().evt_dec_embed(L.ptr(t.emb), L.ptr(t.pe), L.ptr(t.alpha), C.c_float(1.3), L.ptr(yr[b:b + 1]),
                                      L.ptr(ctr), L.ptr(xr[b:b + 1]), 1, t.E, t.ymax, t.npos, L.stream_ptr()),
                "evt_dec_embed")
        torch.cuda.synchronize()
    assert torch.equal(y, yr) and torch.equal(probs, pr) and torch.equal(x, xr)
    st, stop_l, stop_r = rstate.tolist(), stop.tolist(), sr.tolist()
    assert stop_r[5] == t.idx[5] and stop_r[0] == -1            # the reference kernel: EOS at row 5, not at step 0
    for b in range(B):
        before = t.rstate[b]
        if b == 11:
            assert st[b] == before and stop_l[b] == -1 and int(y[b, t.ycount[b]]) == -1
        elif b == 3 and stop_r[b] < 0:
            assert st[b][5] == STOP_LIMIT and stop_l[b] == t.idx[b] and st[b][:5] == before[:5]
        elif stop_r[b] >= 0:
            assert st[b][5] == STOP_EOS and stop_l[b] == stop_r[b] == t.idx[b] and st[b][:5] == before[:5]
        else:
            assert stop_l[b] == -1 and st[b][5] == RUNNING
            assert st[b][:5] == [before[0] + 1, before[1] + 1, before[2] + 1, before[3], before[4]]
    assert st[5][5] == STOP_EOS and st[3][5] in (STOP_LIMIT, STOP_EOS)
    assert len(set(y[b, t.ycount[b]].item() for b in range(B) if b != 11)) > 3
    # ---- a second launch: stopped rows stay, running rows take their next step ----
    y1, x1, st1 = y.clone(), x.clone(), rstate.clone()
    _launch_rows(t, gpu, rstate, y, stop, probs, x)
    for b in range(B):
        if st[b][5] != RUNNING:
            assert torch.equal(rstate[b], st1[b]) and torch.equal(y[b], y1[b]) and torch.equal(x[b], x1[b])
            assert stop.tolist()[b] == stop_l[b]
        elif rstate[b, 5].item() == RUNNING:
            assert rstate[b, 1].item() == t.idx[b] + 2 and int(y[b, t.ycount[b] + 1]) >= 0


def test_dec_sample_embed_rows_mask(gpu):
    """the row mask (step 0 of freshly admitted rows) samples only the chosen rows; dpos = 0 leaves their position"""
    t = _sample_case(gpu, False)
    B = t.B
    rstate, y = _i32(t.rstate, gpu), t.y.to(gpu)
    stop = torch.full((B,), -1, dtype=torch.int32, device=gpu)
    x = torch.full((B, t.E), -7.0, device=gpu)
    chosen = [1, 4, 11]                                          # 11 is idle: chosen, but still skipped
    mask = _i32([1 if b in chosen else 0 for b in range(B)], gpu)
    _launch_rows(t, gpu, rstate, y, stop, None, x, mask=mask, dpos=0)
    st = rstate.tolist()
    for b in range(B):
        if b in (1, 4):
            assert st[b][:3] == [t.rstate[b][0], t.idx[b] + 1, t.ycount[b] + 1] and int(y[b, t.ycount[b]]) >= 0
            assert float(x[b, 0]) != -7.0
        else:
            assert st[b] == t.rstate[b] and int(y[b, t.ycount[b]]) == -1 and float(x[b].max()) == -7.0
    # the same rows in a full launch draw the same tokens
    r2, y2 = _i32(t.rstate, gpu), t.y.to(gpu)
    _launch_rows(t, gpu, r2, y2, torch.full((B,), -1, dtype=torch.int32, device=gpu), None,
                 torch.empty(B, t.E, device=gpu))
    assert all(int(y2[b, t.ycount[b]]) == int(y[b, t.ycount[b]]) for b in (1, 4))


@pytest.fixture(scope="module")
def model(gpu):
    from easevoice_trainer_amd.train.s1_engine import S1Engine

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "gpt.yaml")))
    eng = S1Engine(cfg, gpu, torch.float32)
    fill_module(eng.model, 3)
    eng.model.eval()
    return eng.model


def _refill(m, gpu, d, rows, **kw):
    return m.infer_panel_batch_infer_refill([d["x"][r].to(gpu) for r in rows], d["x_lens"][rows].to(gpu),
                                            d["prompts"][rows].to(gpu), [d["bert"][r].to(gpu) for r in rows], **kw)


def _batch(m, gpu, d, rows, prompts=None, **kw):
    pr = d["prompts"][rows] if prompts is None else prompts
    return m.infer_panel_batch_infer([d["x"][r].to(gpu) for r in rows], d["x_lens"][rows].to(gpu), pr.to(gpu),
                                     [d["bert"][r].to(gpu) for r in rows], **kw)


@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "eager"])
@pytest.mark.parametrize("slots", [8, 32])
def test_refill_matches_reference_tokens(gpu, model, graph, slots, monkeypatch):
    """20 and 36 texts through 8 and through 32 (20) refilled slots: the reference's token lists, fp32"""
    from make_golden_s1_rows import rows_inputs

    monkeypatch.setenv("EVT_DECODE_GRAPH", graph)
    for gold in torch.load(os.path.join(HERE, "golden", "s1_batch_infer_rows.pt"), weights_only=False)["cases"]:
        a = dict(gold["args"])
        R = a.pop("R")
        d = rows_inputs(R)
        ys, idxs = _refill(model, gpu, d, list(range(R)), slots=slots, noise=d["q"], **a)
        assert idxs == gold["idx"], (R, idxs, gold["idx"])
        for r, (y, g) in enumerate(zip(ys, gold["y"])):
            assert torch.equal(y.cpu().long(), g.long()), (R, r)
        st = model._infer().stream_stats
        assert sum(st["admitted"]) == R and st["admissions"] >= (3 if slots == 8 else 1)


def test_refill_seeds_match_the_grouped_path(gpu, model):
    """10 texts under one seed through 5 refilled slots: text for text the tokens of infer_panel_batch_infer(seed) --
    request r draws (seed + 4 * (r // 4), r % 4) in whichever slot and at whichever time it is admitted (every
    group holds the longest text, so the key positions agree)"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(20)
    order = [0, 3, 5, 7, 0, 2, 4, 6, 0, 1]
    kw = dict(top_k=15, top_p=1, early_stop_num=12)
    s = 4242
    ys, idxs = _refill(model, gpu, d, order, slots=5, seed=s, **kw)
    yg, ig = _batch(model, gpu, d, order, seed=s, **kw)
    assert idxs == ig
    for r, (y1, y2) in enumerate(zip(ys, yg)):
        assert torch.equal(y1, y2), r
    assert not torch.equal(ys[0], ys[4])
    assert model._infer().stream_stats["admissions"] >= 2


def test_two_voices_share_a_session(gpu, model):
    """requests alternating between two prompts of different lengths decode in one session; each gets the tokens of
    infer_panel_batch_infer run on its own prompt's group (injected noise columns, fp32; both groups hold the longest
    text)"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(20)
    texts = [0, 0, 3, 5, 7, 2, 4, 6]
    g = torch.Generator().manual_seed(77)
    pa = d["prompts"][0]
    pb = torch.randint(0, 1024, (pa.numel() - 5,), generator=g)
    voice = [pa if i % 2 == 0 else pb for i in range(len(texts))]
    q = d["q"][:, :len(texts)].contiguous()
    kw = dict(top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35, early_stop_num=10)
    reqs = [(d["x"][t].to(gpu), d["bert"][t].to(gpu), voice[i].to(gpu)) for i, t in enumerate(texts)]
    got = {r: (y, i) for r, y, i in model.decode_stream(reqs, slots=3, noise=q, **kw)}
    assert sorted(got) == list(range(len(texts)))
    for v, pr in ((0, pa), (1, pb)):
        members = [i for i in range(len(texts)) if i % 2 == v]
        rows = [texts[i] for i in members]
        ys, idxs = _batch(model, gpu, d, rows, prompts=pr.unsqueeze(0).expand(len(rows), -1).contiguous(),
                          noise=q[:, members].contiguous(), **kw)
        for i, y, idx in zip(members, ys, idxs):
            assert got[i][1] == idx, (i, got[i][1], idx)
            assert torch.equal(got[i][0], y), i
            assert torch.equal(y[:pr.numel()].cpu(), pr)


def test_refill_bf16_repeatable(gpu, model):
    """40 requests through 32 slots in bf16 under one seed: the same tokens twice, all of them valid, every index within
    its limit"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(40)
    model.cd = torch.bfloat16
    try:
        out = [_refill(model, gpu, d, list(range(40)), slots=32, top_k=15, top_p=1, early_stop_num=30, seed=77)
               for _ in range(2)]
        adm = model._infer().stream_stats["admitted"]
    finally:
        model.cd = torch.float32
    (ys1, i1), (ys2, i2) = out
    assert i1 == i2 and len(ys1) == 40 and adm[0] == 32 and sum(adm) == 40
    assert all(torch.equal(a, b) for a, b in zip(ys1, ys2))
    for y, i in zip(ys1, i1):
        assert 0 <= i <= 30 and int(y.min()) >= 0 and int(y[12:].max()) <= 1024 and y.numel() > 12


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def test_synthesize_stream_equals_fragments(gpu):
    """the fragment-by-fragment pipeline gives the waveforms of synthesize_fragments' per-fragment path (speed 1.25,
    tolerance of test_semantic_to_audio_chain), handed out in the order in which the token rows finish: the second
    fragment meets EOS at step 9, the first at step 14"""
    from make_golden_s1_inputs import pipeline_inputs
    from util_fill import decode_inputs
    from easevoice_trainer_amd.auto_reg.t2s_model import Text2SemanticDecoder
    from easevoice_trainer_amd.inference.pipeline import synthesize_fragments, synthesize_stream
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
    kw = dict(top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35, decode_kwargs=dict(noise=dd["noise"].to(gpu)))
    args = (t2s, voice, d["batch_phones"], d["all_ids"], d["bert"], d["prompt"], dd["refers"])
    frags = synthesize_fragments(*args, speed_factor=1.25, sample_kwargs=dict(noise=d["q"]), **kw)
    got = list(synthesize_stream(*args, speed_factor=1.25, sample_kwargs=dict(noise=d["q"], poll=2), **kw))
    assert [i for i, _w in got] == [1, 0]
    finished = [r for kind, _s, r, _slot in t2s.model._infer().stream_stats["events"] if kind == "finish"]
    assert finished == [1, 0]
    for i, w in got:
        assert w.shape == frags[i].shape and rel(w, frags[i]) < 2e-3, (i, rel(w, frags[i]))
